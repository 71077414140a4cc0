"""TEST INFRASTRUCTURE shared by tests/test_forest_diag_host_emu.py (CPU, the numpy emulation) and
tests/test_gpu_forest_diag.py (the device): the host level of the forest diagnostics -- ForestClassifier.out_of_bag,
feature_importances and permutation_importance and the trainer's flags -- against scikit-learn's results recorded by
tests/golden/make_reference_forest_diag.py, against a host loop over the existing predict, and (device only) against the
emulation bit for bit."""
import json
import os
import warnings

import numpy as np
import pytest

from hypelcnn_amd.classic import forest as P
from hypelcnn_amd.classify import classic_ml_trainer as T
from tests import forest_cases as FC
from tests import svm_cases as S

NPZ_PATH = os.path.join(S.GOLDEN, "reference_forest_diag.npz")
_cache = {}


def fixture():
    if "fx" not in _cache:
        _cache["fx"] = dict(np.load(NPZ_PATH))
    return _cache["fx"]


def sk_model(backend, with_impurity=True, with_weight=True):
    fx = fixture()
    return P.ForestClassifier.from_arrays(
        fx["classes"], int(fx["n_features"]), fx["feature"], fx["threshold"], fx["left"], fx["right"], fx["tree_offsets"],
        fx["value"], backend=backend, node_weight=fx["node_weight"] if with_weight else None,
        impurity=fx["impurity"] if with_impurity else None)


def check_sklearn_oob(backend):
    """oob_decision_function_ bit for bit, oob_score_ exactly; every row has a vote; chunked serving changes nothing"""
    fx = fixture()
    m = sk_model(backend)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        score = m.out_of_bag(fx["X"], fx["y"], in_bag_counts=fx["in_bag"])
    assert m.oob_decision_function_.tobytes() == fx["oob_decision_function"].tobytes()
    assert score == m.oob_score_ == float(fx["oob_score"])
    assert np.array_equal(m.oob_votes_, (fx["in_bag"] == 0).sum(0)) and m.oob_votes_.min() > 0
    whole = m.oob_decision_function_.copy()
    m.chunk_rows = 77  # chunks that start at odd rows; ldw stays the full row count
    assert m.out_of_bag(fx["X"], fx["y"], in_bag_counts=fx["in_bag"]) == score
    assert m.oob_decision_function_.tobytes() == whole.tobytes()
    with pytest.raises(ValueError, match="in_bag_counts"):
        m.out_of_bag(fx["X"], fx["y"])
    with pytest.raises(ValueError, match="rows of the training matrix"):
        m.out_of_bag(fx["X"][:100], fx["y"][:100], in_bag_counts=fx["in_bag"])


def importance_bound(fx):
    """2 (F + T) * 2^-53 * the largest importance: every term is non-negative up to rounding, and only the order of the
    two normalising sums and of the mean differs from scikit-learn's (numpy adds pairwise)"""
    f, t = len(fx["feature_importances"]), len(fx["tree_offsets"]) - 1
    return 2 * (f + t) * 2.0 ** -53 * max(fx["feature_importances"].max(), fx["tree_importances"].max())


def check_sklearn_importances(backend):
    """Returns (max |difference| per tree, for the forest).  The stored impurity is scikit-learn's Gini, which the device
    recomputes from `value` when it is not given: both ways stay inside the bound."""
    fx = fixture()
    bound = importance_bound(fx)
    seen = []
    for with_impurity in (True, False):
        m = sk_model(backend, with_impurity)
        imp, rows = m.feature_importances(per_tree=True)
        assert np.array_equal(imp, m.feature_importances()) and m.importances_n_used_ == len(rows) == 20
        per_tree, forest = np.abs(rows - fx["tree_importances"]).max(), np.abs(imp - fx["feature_importances"]).max()
        print(f"impurity {'given' if with_impurity else 'from value'}: max |difference| per tree {per_tree:.3e}, "
              f"forest {forest:.3e}, bound {bound:.3e}")
        if with_impurity:
            assert per_tree <= bound and forest <= bound
        seen.append((per_tree, forest))
    with pytest.raises(ValueError, match="node_weight"):
        sk_model(backend, with_weight=False).feature_importances()
    return seen


def check_permutation_host_loop(backend, model, X, y, group_mod, n_repeats=2, seed=5):
    """hits == a host loop that overwrites the group's columns with X[partner] and calls the existing predict"""
    got = model.permutation_importance(X, y, n_repeats=n_repeats, group_mod=group_mod, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    partners = [rng.permutation(len(X)) for _ in range(n_repeats)]
    f = X.shape[1]
    mod = f if group_mod is None else group_mod
    want = np.zeros((mod, n_repeats), np.int64)
    for g in range(mod):
        cols = np.flatnonzero(np.arange(f) % mod == g)
        for r, partner in enumerate(partners):
            mixed = X.copy()
            mixed[:, cols] = X[partner][:, cols]
            want[g, r] = int((model.predict(mixed) == y).sum())
    assert got["hits"].dtype == np.int64 and np.array_equal(got["hits"], want)
    assert got["baseline"] == float(np.mean(model.predict(X) == y))
    assert np.array_equal(got["importances"], got["baseline"] - want / float(len(X)))
    assert np.array_equal(got["importances_mean"], got["importances"].mean(1))
    assert np.array_equal(got["importances_std"], got["importances"].std(1))
    chunked = model.permutation_importance(X, y, n_repeats=n_repeats, group_mod=group_mod, seed=seed, groups_per_launch=2)
    assert np.array_equal(chunked["hits"], want)  # group windows with g0 > 0
    return got


def grown(kind, backend):
    X, y, _, _ = FC.load("small")
    if kind == "forest":
        return P.ForestClassifier(n_estimators=8, max_features=24, backend=backend).fit(X, y)
    return P.ExtraTreesForest(n_estimators=8, max_features=24, bootstrap=True, backend=backend).fit(X, y)


def three_methods(model, counts=None):
    """(oob score, decision function, votes, importances, per tree, n_used, hits) on the `small` case"""
    X, y, Xv, yv = FC.load("small")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (eight trees: a few rows are in every bag)
        score = model.out_of_bag(X, y, in_bag_counts=counts)
    imp, rows = model.feature_importances(per_tree=True)
    hits = model.permutation_importance(Xv, yv, n_repeats=2, group_mod=9, seed=1)["hits"]
    return score, model.oob_decision_function_, model.oob_votes_, imp, rows, model.importances_n_used_, hits


def check_grown_against_emulation(kind, device_backend, emu_backend):
    """the three methods of a forest grown on the device == the emulation's on the same fitted arrays, bit for bit"""
    m = grown(kind, device_backend)
    twin = type(m).from_arrays(m.classes_, m.n_features_in_, backend=emu_backend, node_weight=m.node_weight_, **m.arrays())
    got, want = three_methods(m), three_methods(twin, m.bootstrap_counts_)
    assert got[0] == want[0] and got[5] == want[5] > 0
    for a, b in zip(got[1:5] + got[6:], want[1:5] + want[6:]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert got[1].any() and got[3].sum() > 0.99 and (got[6] != got[6][0, 0]).any()


REFERENCE_FILES = ("confusion_matrix_SyntheticDataLoader_run0.csv", "metrics_SyntheticDataLoader_run0.txt",
                   "params_SyntheticDataLoader_run0.json")


def check_trainer(make_backend, tmp_path):
    """the three new files with their shapes; the reference's three files byte for byte those of a run without the flags;
    the refusals"""
    path = S.CASES["small_rbf"]["path"]
    common = ["--loader_name", "SyntheticDataLoader", "--path", path, "--neighborhood", "2", "--forest_trees", "8"]
    plain, diag = str(tmp_path / "plain"), str(tmp_path / "diag")
    T.main(["--estimator", "forest", "--base_log_path", plain] + common, backend=make_backend())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = T.main(["--estimator", "forest", "--base_log_path", diag, "--forest_oob", "--forest_importances",
                      "--forest_permutation_repeats", "2"] + common, backend=make_backend())
    est = out[0][0]
    assert sorted(os.listdir(plain)) == sorted(REFERENCE_FILES)
    for name in REFERENCE_FILES:
        assert open(os.path.join(diag, name), "rb").read() == open(os.path.join(plain, name), "rb").read(), name
    p, channels = 5, est.n_features_in_ // 25
    with open(os.path.join(diag, "forest_diagnostics_SyntheticDataLoader_run0.json")) as fh:
        report = json.load(fh)
    assert report["oob_score"] == est.oob_score_ and 0.5 < report["oob_score"] <= 1.0
    assert report["oob_rows_without_vote"] == int((est.oob_votes_ == 0).sum()) and report["n_used"] == 8
    imp = np.load(os.path.join(diag, "feature_importance_SyntheticDataLoader_run0.npy"))
    assert imp.shape == (p, p, channels) and imp.dtype == np.float64 and abs(imp.sum() - 1.0) < 1e-12
    assert np.array_equal(imp.reshape(-1), est.feature_importances())
    with open(os.path.join(diag, "band_importance_SyntheticDataLoader_run0.csv")) as fh:
        lines = fh.read().splitlines()
    assert lines[0] == "band,impurity_importance,permutation_mean,permutation_std" and len(lines) == channels + 1
    table = np.array([[float(v) for v in line.split(",")] for line in lines[1:]])
    assert np.array_equal(table[:, 0], np.arange(channels)) and np.array_equal(table[:, 1], imp.sum((0, 1)))
    assert np.isfinite(table).all() and (table[:, 3] >= 0).all()
    assert len(os.listdir(diag)) == 6

    only = str(tmp_path / "only_oob")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        T.main(["--estimator", "forest", "--base_log_path", only, "--forest_oob"] + common, backend=make_backend())
    assert sorted(os.listdir(only)) == sorted(REFERENCE_FILES + ("forest_diagnostics_SyntheticDataLoader_run0.json",))
    with pytest.raises(ValueError, match="Out of bag estimation only available if bootstrap=True"):
        T.main(["--estimator", "extra_trees", "--forest_oob", "--base_log_path", str(tmp_path / "x")] + common,
               backend=make_backend())
    for flag in (["--forest_oob"], ["--forest_importances"], ["--forest_permutation_repeats", "1"]):
        with pytest.raises(ValueError, match="forest"):
            T.main(["--estimator", "svc_rbf", "--base_log_path", str(tmp_path / "y")] + flag + common,
                   backend=make_backend())
    assert not os.path.exists(str(tmp_path / "y"))  # refused before anything is fitted or written
