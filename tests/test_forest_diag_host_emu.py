"""CPU: ForestClassifier.out_of_bag, feature_importances and permutation_importance and the trainer's --forest_oob,
--forest_importances and --forest_permutation_repeats on the numpy emulation of the three entry points
(tests/emu_forest.py), against scikit-learn 1.7.2's RandomForestClassifier(oob_score=True) recorded by
tests/golden/make_reference_forest_diag.py and against a host loop over the existing predict.
tests/test_gpu_forest_diag.py runs the same checks on the device."""
import warnings

import numpy as np
import pytest

from hypelcnn_amd.classic import forest as P
from tests import emu_forest, emu_scene  # noqa: F401 -- attach the emulations
from tests import forest_cases as FC
from tests import forest_diag_checks as H
from tests.emu_backend import EmuBackend


def test_fixture_is_the_makers_problem_and_small():
    import os
    from tests.golden import make_reference_forest_diag as M
    fx = H.fixture()
    X, y = M.problem()
    assert X.shape == (300, 12) and X.dtype == np.float32 and len(np.unique(y)) == 5
    assert np.array_equal(fx["X"], X) and np.array_equal(fx["y"], y) and str(fx["sklearn"]) == "1.7.2"
    assert len(fx["tree_offsets"]) == 21 and fx["in_bag"].shape == (20, 300) and (fx["in_bag"].sum(1) == 300).all()
    assert os.path.getsize(H.NPZ_PATH) <= os.path.getsize(FC.NPZ_PATH)


def test_out_of_bag_equals_scikit_learn_bit_for_bit():
    H.check_sklearn_oob(EmuBackend())


def test_feature_importances_within_the_summation_bound_of_scikit_learn():
    """The bound is 2 * (12 + 20) * 2^-53 * the largest importance = 2.9e-15.  Observed on the emulation with the stored
    impurity: at most 5.6e-17 per tree, 1.1e-16 for the forest (with Gini recomputed from value, which the bound does not
    speak about and which is printed only: 2.8e-16 and 5.6e-17)."""
    H.check_sklearn_importances(EmuBackend())


@pytest.mark.parametrize("group_mod", [None, 9, 4])
def test_permutation_importance_equals_a_host_loop_over_predict(group_mod):
    be = EmuBackend()
    _, _, Xv, yv = FC.load("small")
    if group_mod is None:
        H.check_permutation_host_loop(be, _narrow(be), Xv[:, :36], yv, None)
    else:  # 9: the channel count of the patch; 4 does not divide the 225 columns
        H.check_permutation_host_loop(be, _fitted(be), Xv, yv, group_mod)


_models = {}


def _fitted(be):
    if "small" not in _models:
        _models["small"] = H.grown("forest", be)
    return _models["small"]


def _narrow(be):
    """36 columns: every column its own group stays a short host loop"""
    if "narrow" not in _models:
        X, y, _, _ = FC.load("small")
        _models["narrow"] = P.ForestClassifier(n_estimators=4, max_features=6, backend=be).fit(X[:, :36], y)
    return _models["narrow"]


def test_out_of_bag_of_grown_forests_and_its_errors():
    be = EmuBackend()
    X, y, _, _ = FC.load("small")
    m = _fitted(be)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        score = m.out_of_bag(X, y)
    votes = (m.bootstrap_counts_ == 0).sum(0)
    assert np.array_equal(m.oob_votes_, votes) and m.oob_decision_function_.shape == (len(y), len(m.classes_))
    some = votes > 0
    assert np.allclose(m.oob_decision_function_[some].sum(1), 1.0) and not m.oob_decision_function_[~some].any()
    labels = m.classes_[np.argmax(m.oob_decision_function_, 1)]
    assert score == m.oob_score_ == float(np.mean(labels == y)) and 0.5 < score < 1.0
    full = m.predict_proba(X)
    never = P.ForestClassifier.from_arrays(m.classes_, m.n_features_in_, backend=be, **m.arrays())
    never.out_of_bag(X, y, in_bag_counts=np.zeros_like(m.bootstrap_counts_))  # no row in any bag: the served means
    assert never.oob_decision_function_.tobytes() == full.tobytes() and (never.oob_votes_ == m.n_estimators).all()
    two = P.ForestClassifier(n_estimators=2, max_features=24, backend=be).fit(X, y)
    with pytest.warns(UserWarning, match="in every tree's bag"):
        two.out_of_bag(X, y)
    assert (two.oob_votes_ == 0).any()
    for kind in (P.ExtraTreesForest(n_estimators=2, backend=be), P.ForestClassifier(n_estimators=2, bootstrap=False, backend=be)):
        with pytest.raises(ValueError, match="Out of bag estimation only available if bootstrap=True"):
            kind.fit(X, y).out_of_bag(X, y)
    et = H.grown("extra_trees", be)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert 0.5 < et.out_of_bag(X, y) <= 1.0


def test_feature_importances_of_grown_forests():
    be = EmuBackend()
    for kind in ("forest", "extra_trees"):
        m = _fitted(be) if kind == "forest" else H.grown(kind, be)
        imp, rows = m.feature_importances(per_tree=True)
        assert imp.shape == (m.n_features_in_,) and rows.shape == (8, m.n_features_in_) and m.importances_n_used_ == 8
        assert abs(imp.sum() - 1.0) < 1e-12 and np.allclose(rows.sum(1), 1.0) and (imp >= 0).all()
        never_split = np.setdiff1d(np.arange(m.n_features_in_), m.feature_[m.feature_ >= 0])
        assert not imp[never_split].any() and (imp[np.unique(m.feature_[m.feature_ >= 0])] > 0).any()
    stumps = P.ForestClassifier(n_estimators=3, max_depth=0, backend=be).fit(*FC.load("small")[:2])
    assert not stumps.feature_importances().any() and stumps.importances_n_used_ == 0
    assert m.get_params() == H.grown("extra_trees", be).get_params()  # the diagnostics are methods, no parameters


def test_trainer_writes_the_three_files_and_keeps_the_reference_files(tmp_path):
    H.check_trainer(EmuBackend, tmp_path)
