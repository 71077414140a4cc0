"""-m gpu: the extra-trees kernels of csrc/forest.hip through the C-ABI (HipBackend.call), one entry point at a time,
against the brute-force reference of tests/extra_trees_kernel_cases.py -- plain Python written from include/hypel.h, not
the numpy emulation the host-level suite (tests/test_gpu_extra_trees.py) compares with.
tests/test_extra_trees_kernel_cases_emu.py runs the same cases through the emulation on the CPU and shows that planted
defects are rejected.

Every operand lies at an odd element offset inside sentinel bytes; every launch runs twice and must write the same bytes;
after it every byte of every operand, inputs and the unspecified parts of the outputs included, must equal what the
reference left.  All comparisons are equalities of bytes or integers."""
import pytest

from tests import extra_trees_kernel_cases as X
from tests import forest_kernel_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.mark.parametrize("n,f", X.COLUMN_CASES)
def test_x1_columns(hip, n, f):
    """both zeros in one column come out +0.0; row tails and the column past the last keep the sentinel"""
    X.run_columns(hip, n, f)


@pytest.mark.parametrize("name", list(X.RANDOM_CASES))
def test_x2_split_random(hip, name):
    """row counts 1 .. 1000, 2 and 32 classes, weights above 1, max_features 1 and f, 600 nodes of 2 .. 8 rows"""
    X.run_random(hip, name)


def test_x2_split_random_special_columns(hip):
    """constant, both zeros, -FLT_MAX .. FLT_MAX, one denormal, all but one row left, one ulp with the largest u"""
    X.run_random_special(hip)


def test_x3_split_apply_thr_partition(hip):
    K.run_partition(hip, K.CUTS)


@pytest.mark.parametrize("level,max_depth", K.LEAF_LEVELS)
def test_x3_split_apply_thr_leaf_reasons(hip, level, max_depth):
    K.run_leaf_reasons(hip, K.CUTS, level, max_depth)


def test_x3_split_apply_thr_slot_ties(hip):
    K.run_slot_ties(hip, K.CUTS)


@pytest.mark.parametrize("n_active", K.COMPACT_N)
def test_x3_split_apply_thr_compaction(hip, n_active):
    for pattern in K.COMPACT_PATTERNS:
        K.run_compaction(hip, K.CUTS, n_active, pattern)
    K.run_compaction(hip, K.CUTS, n_active, "alternating", short=1)
    K.run_compaction(hip, K.CUTS, n_active, "last", short=1)


@pytest.mark.parametrize("name", ["600_nodes", "c32_mff"])
def test_x3_split_random_then_apply(hip, name):
    X.run_random_then_apply(hip, name)


def test_x4_refusals_leave_every_byte(hip):
    X.run_refusals(hip)
