"""-m gpu: the seven kernels of csrc/forest.hip through the C-ABI (HipBackend.call), one entry point at a time, against
the brute-force reference of tests/forest_kernel_cases.py -- plain Python written from include/hypel.h, not the numpy
emulation the host-level suite (tests/test_gpu_forest.py) compares with.  The case module holds the tables, the operand
windows and the reference; tests/test_forest_kernel_cases_emu.py runs the same cases through the emulation on the CPU and
shows that planted defects and stray writes are rejected.

Every operand lies at an odd element offset inside sentinel bytes, row operands with ld > f and the bins with ldn > n; every
launch runs twice and must write the same bytes; after it every byte of every operand, inputs and the unspecified parts
of the outputs included, must equal what the reference left.  All comparisons are equalities of bytes or integers."""
import pytest

from tests import forest_kernel_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.mark.parametrize("k,case", list(enumerate(K.BIN_CASES)), ids=[f"{n}x{b}" for n, b in K.BIN_CASES])
def test_f1_bin_edges_and_bins(hip, k, case):
    """forest_kernel_cases.run_bins: edges and n_edges of five kinds of column through a non-identity permutation, the
    bins of the same rows and of probe rows on and one ulp beside every edge; bin <= t <=> x <= edges[c][t]"""
    K.run_bins(hip, *case, k)


@pytest.mark.parametrize("name", list(K.HIST_CASES))
def test_f2_split_hist(hip, name):
    """forest_kernel_cases.run_hist: score, best_bin and valid of every record, the records past the last untouched"""
    K.run_hist(hip, name)


def test_f3_split_apply_partition(hip):
    """counts 2 .. 1000 with one row, all but one and a random number going left: the order element by element"""
    K.run_partition(hip, K.BINS)


@pytest.mark.parametrize("level,max_depth", K.LEAF_LEVELS)
def test_f3_split_apply_leaf_reasons(hip, level, max_depth):
    K.run_leaf_reasons(hip, K.BINS, level, max_depth)


def test_f3_split_apply_slot_ties(hip):
    K.run_slot_ties(hip, K.BINS)


@pytest.mark.parametrize("n_active", K.COMPACT_N)
def test_f3_split_apply_compaction(hip, n_active):
    """all, none, every other and only the last node split; node_capacity exact, and one too small (counter = -1)"""
    for pattern in K.COMPACT_PATTERNS:
        K.run_compaction(hip, K.BINS, n_active, pattern)
    K.run_compaction(hip, K.BINS, n_active, "alternating", short=1)
    K.run_compaction(hip, K.BINS, n_active, "last", short=1)


@pytest.mark.parametrize("name", ["c2_mf1", "heavy_c32", "special"])
def test_f3_split_hist_then_apply(hip, name):
    K.run_hist_then_apply(hip, name)


@pytest.mark.parametrize("n,n_classes,n_trees", K.PREDICT_CASES)
def test_f4_predict_rows(hip, n, n_classes, n_trees):
    """stumps, 64-deep chains and balanced trees; class_labels, points and proba present and NULL"""
    K.run_predict(hip, n, n_classes, n_trees)


def test_f4_predict_rows_ties_and_thresholds(hip):
    K.run_predict_ties(hip)
    K.run_predict_threshold(hip)


@pytest.mark.parametrize("p,cc,cl,n", K.SCENE_CASES)
def test_f5_predict_scene(hip, p, cc, cl, n):
    """the four corners of the padded scene; the reference, and hypel_forest_predict_rows on the gather kernel's patches"""
    K.run_scene(hip, p, cc, cl, n)


def test_f6_refusals_leave_every_byte(hip):
    K.run_refusals(hip)
