"""-m gpu: the forest diagnostics of csrc/forest.hip through the C-ABI (HipBackend.call), one entry point at a time,
against the brute-force reference of tests/forest_diag_cases.py -- plain Python written from include/hypel.h, not the
numpy emulation.  tests/test_forest_diag_emu.py runs the same cases through the emulation on the CPU and shows that
planted defects are rejected.  Every operand lies at an odd element offset inside sentinel bytes; every launch runs twice
and must write the same bytes; after it every byte of every operand, inputs and the unspecified parts of the outputs
included, must equal what the reference left.

Then the host level on the device (tests/forest_diag_checks.py): scikit-learn's recorded out-of-bag decision function bit
for bit, its importances within the summation bound, permutation hits against a host loop over predict, the trainer's
files, and the three methods of a grown ForestClassifier and a grown ExtraTreesForest(bootstrap=True) against the
emulation bit for bit."""
import pytest

from tests import emu_forest, emu_scene  # noqa: F401 -- attach the emulations
from tests import forest_cases as FC
from tests import forest_diag_cases as D
from tests import forest_diag_checks as H
from tests.emu_backend import EmuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.mark.parametrize("n,n_classes,n_trees", D.OOB_CASES)
def test_d1_oob_rows(hip, n, n_classes, n_trees):
    """a row in every bag (votes 0, zeros, class 0), a row in no bag (the served means), counts above 1, ldw > n from an
    odd row of the table"""
    D.run_oob(hip, n, n_classes, n_trees)


@pytest.mark.parametrize("case", D.HIT_CASES)
def test_d2_permuted_hits(hip, case):
    """group_mod 1, f, 4 (not a divisor of 6) and 8 (groups without a column); the identity partner; windows at g0 > 0"""
    D.run_hits(hip, *case)


@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("f", D.IMPORTANCE_F)
def test_d3_importances(hip, f, given):
    """one window and two; a claim chain longer than the block; interleaved columns over three chunks; a lone root; a
    tree of zero decreases"""
    D.run_importances(hip, f, given)


def test_d3_importances_lone_roots(hip):
    D.run_importances_lone_roots(hip)


def test_d4_refusals_leave_every_byte(hip):
    D.run_refusals(hip)


def test_h1_out_of_bag_equals_scikit_learn_bit_for_bit(hip):
    H.check_sklearn_oob(hip)


def test_h2_feature_importances_within_the_summation_bound_of_scikit_learn(hip):
    """bound 2.9e-15; the device repeats the emulation's figures (tests/test_forest_diag_host_emu.py): 5.6e-17 per tree,
    1.1e-16 for the forest"""
    assert H.check_sklearn_importances(hip) == H.check_sklearn_importances(EmuBackend())


@pytest.mark.parametrize("group_mod", [9, 4])
def test_h3_permutation_importance_equals_a_host_loop_over_predict(hip, group_mod):
    _, _, Xv, yv = FC.load("small")
    H.check_permutation_host_loop(hip, _fitted(hip), Xv, yv, group_mod)


_models = {}


def _fitted(hip):
    if "small" not in _models:
        _models["small"] = H.grown("forest", hip)
    return _models["small"]


@pytest.mark.parametrize("kind", ["forest", "extra_trees"])
def test_h4_grown_forests_equal_the_emulation_bit_for_bit(hip, kind):
    H.check_grown_against_emulation(kind, hip, EmuBackend())


def test_h5_trainer_writes_the_three_files(hip, tmp_path):
    H.check_trainer(lambda: hip, tmp_path)
