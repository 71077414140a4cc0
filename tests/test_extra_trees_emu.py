"""CPU: hypelcnn_amd.classic.forest.ExtraTreesForest and `classic_ml_trainer --estimator extra_trees` on the numpy
emulation of the extra-trees entry points (tests/emu_forest.py): purity, seeds, a brute-force fit that replays the
documented draw order, the trainer, and the accuracy against scikit-learn's ExtraTreesClassifier recorded by
tests/golden/make_reference_extra_trees.py.  tests/test_gpu_extra_trees.py holds the device to this emulation bit for
bit."""
import json
import os

import numpy as np
import pytest

from hypelcnn_amd.classic import forest as P
from hypelcnn_amd.classify import classic_ml_trainer as T
from tests import emu_forest, emu_scene  # noqa: F401 -- attach the emulations to EmuBackend
from tests import extra_trees_cases as XC
from tests import forest_cases as FC
from tests import svm_cases as S
from tests.emu_backend import EmuBackend

_fitted = {}


def fitted(case="small", **kw):
    """the case's eight trees (forest_cases.CASES), fitted once per module and argument set"""
    key = (case, tuple(sorted(kw.items())))
    if key not in _fitted:
        X, y, _, _ = FC.load(case)
        args = dict(FC.CASES[case][1])
        args.update(kw)
        _fitted[key] = XC.recording_extra_trees()(backend=EmuBackend(), **args).fit(X, y)
    return _fitted[key]


def check_purity(m, X, y):
    """no depth cap was met, so every leaf holds one class: the training rows come back exactly"""
    assert m.n_levels_ <= P.FOREST_MAX_DEPTH and not m.bootstrap
    assert np.array_equal(m.predict(X), y)
    leaves = m.value_[m.left_ < 0]
    assert ((leaves == 0) | (leaves == 1)).all() and (leaves.sum(1) == 1).all()
    assert (m.threshold_bin_ == -1).all() and len(m.threshold_bin_) == len(m.feature_)
    assert (m.node_weight_ == m.node_count_).all()


def test_trees_are_pure_without_bootstrap():
    X, y, _, _ = FC.load("small")
    m = fitted()
    check_purity(m, X, y)
    assert m.n_estimators == 8 and m.get_params() == {"bootstrap": False, "max_depth": None, "max_features": 24,
                                                      "n_estimators": 8, "seed": 0}
    json.dumps(m.get_params())
    with pytest.raises(TypeError):
        P.ExtraTreesForest(n_bins=256)


def test_seeds_and_bootstrap():
    X, y, _, _ = FC.load("small")
    a = fitted()
    b = XC.recording_extra_trees()(backend=EmuBackend(), **FC.CASES["small"][1]).fit(X, y)
    XC.same_arrays(a.arrays(), b.arrays(), "the same seed")
    c = fitted(seed=1)
    assert len(c.feature_) != len(a.feature_) or not np.array_equal(c.threshold_, a.threshold_)
    d = fitted(bootstrap=True)
    assert (a.bootstrap_counts_ == 1).all() and (d.bootstrap_counts_ != 1).any()
    assert (d.bootstrap_counts_.sum(1) == len(y)).all()
    assert len(d.feature_) != len(a.feature_) or not np.array_equal(d.threshold_, a.threshold_)


@pytest.mark.parametrize("kw", [dict(), dict(bootstrap=True, seed=3), dict(max_depth=3), dict(max_features=None)],
                         ids=["default", "bootstrap", "depth3", "every_column"])
def test_fit_equals_the_brute_force_fit(kw):
    X, y, _, _ = FC.load("small")
    args = dict(n_estimators=3, max_features=24, seed=0)
    args.update(kw)
    m = P.ExtraTreesForest(backend=EmuBackend(), **args).fit(X, y)
    brute = dict(args)
    brute["max_features"] = X.shape[1] if args["max_features"] is None else args["max_features"]
    want, levels = XC.brute_fit(X, y, **brute)
    XC.same_arrays(m.arrays(), want, kw)
    assert m.n_levels_ == levels and (kw.get("max_depth") is None or levels == 4)


def test_served_from_arrays_equals_the_fitted_model():
    m = fitted()
    _, _, Xv, _ = FC.load("small")
    served = P.ExtraTreesForest.from_arrays(m.classes_, m.n_features_in_, backend=EmuBackend(), **m.arrays())
    assert isinstance(served, P.ExtraTreesForest)
    assert np.array_equal(served.predict_proba(Xv), m.predict_proba(Xv))


def test_cli_end_to_end_and_refusals(tmp_path):
    path = S.CASES["small_rbf"]["path"]
    common = ["--loader_name", "SyntheticDataLoader", "--path", path, "--neighborhood", "2"]
    out = T.main(["--estimator", "extra_trees", "--forest_trees", "8", "--forest_bins", "7", "--fullscene",
                  "--base_log_path", str(tmp_path / "log"), "--output_path", str(tmp_path / "out")] + common,
                 backend=EmuBackend())
    est, predicted, cm, (oa, _, _), scene = out[0]
    assert isinstance(est, P.ExtraTreesForest) and est.n_estimators == 8 and est.seed == 0 and not est.bootstrap
    XC.same_arrays(est.arrays(), fitted().arrays(), "the CLI's defaults = the case")
    for name in ("confusion_matrix_SyntheticDataLoader_run0.csv", "metrics_SyntheticDataLoader_run0.txt",
                 "params_SyntheticDataLoader_run0.json"):
        assert os.path.getsize(tmp_path / "log" / name) > 0
    with open(tmp_path / "log" / "params_SyntheticDataLoader_run0.json") as f:
        assert json.load(f) == est.get_params()
    for name in ("result_raw.tif", "result_colorized.tif"):
        assert os.path.getsize(tmp_path / "out" / name) > 0
    rows, (h, w) = S.load_scene_rows("small_rbf")
    assert np.array_equal(scene, est.predict(rows).reshape(h, w)) and oa == np.trace(cm) / cm.sum()
    assert len(np.unique(scene)) > 1
    assert "extra_trees" in T.ESTIMATORS and T.create_estimator(T.build_parser().parse_known_args(
        ["--estimator", "extra_trees", "--forest_seed", "3"])[0], EmuBackend(), run_index=2).seed == 5
    with pytest.raises(ValueError, match="svc_grid"):
        T.main(["--estimator", "extra_trees", "--svc_grid"] + common, backend=EmuBackend())
    with pytest.raises(NotImplementedError, match="extra_trees"):
        T.main(["--estimator", "ExtraTreesClassifier"] + common, backend=EmuBackend())


def test_predict_scene_equals_predict_on_both_paths():
    import torch
    model = fitted()
    rows, (h, w) = S.load_scene_rows(FC.CASES["small"][0])
    want = model.predict(rows).astype(np.uint8).reshape(h, w)
    arrays, _ = FC.scene_arrays("small", model._backend())
    for direct in (True, False):
        raster = torch.zeros(h * w, dtype=torch.uint8)
        model.predict_scene(arrays, raster, w, direct=direct)
        assert np.array_equal(raster.numpy().reshape(h, w), want), direct


def accuracy_bound(fx):
    """the recorded scikit-learn mean minus two binomial standard errors of ONE run on the 800 validation rows: sampling
    noise of the validation set and nothing else"""
    p = float(fx["sk_oa"].mean())
    return p, p - 2.0 * np.sqrt(p * (1.0 - p) / len(fx["y_val"]))


def mean_accuracy(backend):
    fx = XC.load_fixture()
    oa = [float((P.ExtraTreesForest(30, max_features=5, seed=s, backend=backend).fit(fx["X_train"], fx["y_train"])
                 .predict(fx["X_val"]) == fx["y_val"]).mean()) for s in range(6)]
    return oa


def test_accuracy_is_scikit_learns_within_sampling_noise():
    fx = XC.load_fixture()
    assert fx["X_train"].shape == (400, 30) and fx["X_val"].shape == (800, 30) and fx["X_train"].dtype == np.float32
    assert len(np.unique(fx["y_train"])) == 5 and len(fx["sk_oa"]) == 6
    p, bound = accuracy_bound(fx)
    oa = mean_accuracy(EmuBackend())
    print(f"ExtraTreesForest {oa}, mean {np.mean(oa):.4f}; scikit-learn mean {p:.4f}, bound {bound:.4f}")
    assert np.mean(oa) >= bound
