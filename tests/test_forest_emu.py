"""CPU: hypelcnn_amd.classic.forest.ForestClassifier and `classic_ml_trainer --estimator forest` on the numpy emulation
of the hypel_forest_* entry points (tests/emu_forest.py), against the scikit-learn fixture of
tests/golden/make_reference_forest.py.  tests/test_gpu_forest.py holds the device to this emulation bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from hypelcnn_amd.classic import forest as P
from hypelcnn_amd.classify import classic_ml_trainer as T
from tests import emu_forest, emu_scene  # noqa: F401 -- attach the emulations to EmuBackend
from tests import forest_cases as FC
from tests import svm_cases as S
from tests.emu_backend import EmuBackend


@pytest.fixture(scope="module")
def fixture():
    return FC.load_fixture()


_fitted = {}


def fitted(case):
    """the case's forest, unbounded, every level recorded; fitted once per module"""
    if case not in _fitted:
        X, y, _, _ = FC.load(case)
        m = FC.make(case, EmuBackend())
        m.record_levels = P.FOREST_MAX_DEPTH + 1
        _fitted[case] = m.fit(X, y)
    return _fitted[case]


def _bins(model, n):
    return model._bins.numpy().reshape(-1, model._ldn)[:, :n].T


def _node_rows(model, X_bins, rows_in_bag, tree):
    """model node -> the in-bag rows that reach it (walk on the bin matrix)"""
    lo, hi = model.tree_offsets_[tree], model.tree_offsets_[tree + 1]
    reach = {int(lo): rows_in_bag}
    for node in range(lo, hi):  # a child's number exceeds its parent's
        if model.left_[node] < 0:
            continue
        rows = reach[node]
        go = X_bins[rows, model.feature_[node]] <= model.threshold_bin_[node]
        reach[int(lo + model.left_[node])], reach[int(lo + model.right_[node])] = rows[go], rows[~go]
    return reach


# 1 ---------------------------------------------------------------------------------------------------------------
def test_single_tree_equals_scikit_learn_on_the_bins(fixture):
    meta, fx = fixture
    X, y = FC.load_tree_case()  # `small` with another seed and six classes: see forest_cases.TREE_PATH
    m = FC.make("small", EmuBackend(), n_estimators=1, bootstrap=False, max_features=None, max_depth=6).fit(X, y)
    assert meta["tree"]["max_depth"] == meta["tree"]["max_depth_asked"] == 6 and meta["tree"]["identical"]
    assert meta["tree"]["path"] == FC.TREE_PATH and meta["tree"]["tree_depth"] == 4
    t = {k: fx[f"small/tree/{k}"] for k in ("feature", "left", "right", "left_max_bin", "n_node_samples", "leaf_class")}
    pairs, seen = [(0, 0)], 0  # (fixture node, model node): the fixture numbers depth-first, the model breadth-first
    while pairs:
        a, b = pairs.pop()
        seen += 1
        assert m.node_count_[b] == t["n_node_samples"][a]
        if t["left"][a] < 0:  # scikit-learn's tree ends above the depth cap, so its leaves are leaves here too
            assert m.left_[b] < 0 and np.argmax(m.value_[b]) == t["leaf_class"][a]
            continue
        assert m.feature_[b] == t["feature"][a] and m.threshold_bin_[b] == t["left_max_bin"][a]
        pairs += [(t["left"][a], m.left_[b]), (t["right"][a], m.right_[b])]
    assert seen == meta["tree"]["node_count"] == len(m.feature_)
    # every split of the depth-6 tree is the greedy optimum with the header's tie rule, recomputed with sorted columns
    # and cumulative sums over the whole bin matrix at once (no histogram, no candidate table)
    B = _bins(m, len(y)).astype(np.int64)
    cls = np.searchsorted(m.classes_, y)
    onehot = np.eye(len(m.classes_), dtype=np.int64)[cls]
    reach = _node_rows(m, B, np.arange(len(y)), 0)
    assert (m.left_ >= 0).sum() >= 5
    for node in np.flatnonzero(m.left_ >= 0):
        rows = reach[int(node)]
        best = (-1.0, -1, -1)
        for c in range(B.shape[1]):
            order = np.argsort(B[rows, c], kind="stable")
            b_sorted = B[rows, c][order]
            cut = np.flatnonzero(np.diff(b_sorted) > 0)  # the left side ends at sorted position cut
            if not len(cut):
                continue
            L = np.cumsum(onehot[rows][order], 0)[cut]
            R = onehot[rows].sum(0)[None, :] - L
            sc = (L * L).sum(1) / L.sum(1) + (R * R).sum(1) / R.sum(1)
            k = int(np.argmax(sc))
            if sc[k] > best[0]:
                best = (float(sc[k]), c, int(b_sorted[cut[k]]))
        assert (m.feature_[node], m.threshold_bin_[node]) == best[1:], (node, best)
        assert m.threshold_[node] == m._edges.numpy().reshape(-1, P.FOREST_MAX_EDGES)[best[1], best[2]]


# 2 ---------------------------------------------------------------------------------------------------------------
def test_fit_is_deterministic_and_seeded():
    X, y, _, _ = FC.load("small")
    a = fitted("small")
    b = FC.make("small", EmuBackend()).fit(X, y)
    for k, v in a.arrays().items():
        assert np.array_equal(v, b.arrays()[k]), k
    c = FC.make("small", EmuBackend(), seed=1).fit(X, y)
    assert len(c.feature_) != len(a.feature_) or not np.array_equal(c.feature_, a.feature_)
    assert a.get_params() == {"bootstrap": True, "max_depth": None, "max_features": 24, "n_bins": 256, "n_estimators": 8,
                              "seed": 0}
    json.dumps(a.get_params())


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "small_edges"])
def test_every_leaf_is_pure_single_or_without_valid_candidate(case):
    X, y, _, _ = FC.load(case)
    m = fitted(case)
    B = _bins(m, len(y))
    cls = np.searchsorted(m.classes_, y)
    cand_of = {}
    for active, cand, _, _, _ in m.level_records_:
        for rec, cd in zip(active, cand):
            cand_of[int(m.model_node_[rec[3]])] = cd
    assert len(cand_of) == len(m.feature_) and m.n_levels_ <= P.FOREST_MAX_DEPTH
    kinds = {"pure": 0, "single": 0, "no_candidate": 0}
    for tree in range(m.n_estimators):
        in_bag = np.flatnonzero(m.bootstrap_counts_[tree] > 0)
        reach = _node_rows(m, B, in_bag, tree)
        for node in range(m.tree_offsets_[tree], m.tree_offsets_[tree + 1]):
            rows = reach[node]
            assert len(rows) == m.node_count_[node] >= 1
            assert m.bootstrap_counts_[tree][rows].sum() == m.node_weight_[node]
            w = np.bincount(cls[rows], weights=m.bootstrap_counts_[tree][rows], minlength=len(m.classes_))
            assert np.array_equal(m.value_[node], w / w.sum())
            if m.left_[node] >= 0:
                continue
            if len(np.unique(cls[rows])) == 1:
                kinds["pure"] += 1
            elif len(rows) == 1:
                kinds["single"] += 1
            else:  # every candidate column keeps the node's rows in one bin
                assert all(len(np.unique(B[rows, c])) == 1 for c in cand_of[node]), (tree, node)
                kinds["no_candidate"] += 1
    print(case, kinds)
    assert kinds["pure"] > 0


# 4 ---------------------------------------------------------------------------------------------------------------
def test_planted_tie_goes_to_the_lower_feature_and_planted_columns_behave():
    m = fitted("small_edges")
    assert m._resolve_max_features(225) == 225  # max_features=300 is clamped to F
    ne = m._n_edges.numpy()
    assert ne[FC.CONSTANT_COL] == 0 and ne[FC.THREE_COL] == 2
    assert not (m.feature_ == FC.CONSTANT_COL).any()
    active, cand, score, best_bin, valid = m.level_records_[0]
    score, best_bin, valid = (v.reshape(cand.shape) for v in (score, best_bin, valid))
    for a in range(len(active)):
        lo, hi = np.flatnonzero(cand[a] == FC.TIE_LOW)[0], np.flatnonzero(cand[a] == FC.TIE_HIGH)[0]
        assert valid[a, lo] and valid[a, hi] and score[a, lo] == score[a, hi] and best_bin[a, lo] == best_bin[a, hi]
        assert not valid[a, np.flatnonzero(cand[a] == FC.CONSTANT_COL)[0]]
        assert score[a, lo] == score[a].max()  # the tie IS the best score, so the rule decides the root
    assert (m.feature_[m.tree_offsets_[:-1]] == FC.TIE_LOW).all()
    assert not (m.feature_ == FC.TIE_HIGH).any()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small", "grss2013"])
def test_validation_accuracy_within_scikit_learns_own_spread(case, fixture):
    meta, _ = fixture
    c = meta["cases"][case]
    _, _, Xv, yv = FC.load(case)
    assert c["oa_bound"] == min(c["oa"]) - max(max(c["oa"]) - min(c["oa"]), 2.0 / c["n_val"]) and c["n_val"] == len(yv)
    oa = float((fitted(case).predict(Xv) == yv).mean())
    print(f"{case}: OA {oa:.4f}, bound {c['oa_bound']:.4f}, scikit-learn {min(c['oa']):.4f}..{max(c['oa']):.4f}")
    assert oa >= c["oa_bound"]


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def served(fixture):
    _, fx = fixture
    return {case: P.ForestClassifier.from_arrays(backend=EmuBackend(), **FC.sk_arrays(fx, case))
            for case in ("small", "grss2013")}


@pytest.mark.parametrize("case", ["small", "grss2013"])
def test_served_scikit_learn_forest_gives_its_labels(case, fixture, served):
    _, fx = fixture
    _, _, Xv, _ = FC.load(case)
    k = f"{case}/rf/"
    model = served[case]
    assert model.n_estimators == FC.SK_TREES and model.threshold_.dtype == np.float32
    FC.check_served_labels(model.predict(Xv), fx[k + "proba_validation"], fx[k + "predict_validation"], case)
    assert np.array_equal(model.predict_proba(Xv), fx[k + "proba_validation"])  # the same fp64 sums in the same order
    if case == "small":
        rows, _ = S.load_scene_rows(FC.CASES[case][0])
        FC.check_served_labels(model.predict(rows), fx[k + "proba_scene"], fx[k + "predict_scene"], case + "/scene")


def test_float64_thresholds_round_down():
    thr = np.array([0.1, 1.0, -0.1, 1e-50, 3.0000001])
    t32 = P.round_down_f32(thr)
    assert t32.dtype == np.float32 and (t32.astype(np.float64) <= thr).all()
    assert (np.nextafter(t32, np.float32(np.inf)).astype(np.float64) > thr).all()
    # the case plain rounding gets wrong: x is the float32 just above the threshold and the threshold rounds up to it
    x = np.float32(0.1)
    assert np.float64(x) > 0.1 and np.float32(0.1) == x and not x <= t32[0]
    X = np.array([[x], [np.nextafter(x, np.float32(0))]], np.float32)
    m = P.ForestClassifier.from_arrays([0, 1], 1, [0, -1, -1], np.array([0.1, 0, 0]), [1, -1, -1], [2, -1, -1], [0, 3],
                                       [[.5, .5], [1, 0], [0, 1]], backend=EmuBackend())
    assert m.predict(X).tolist() == [1, 0]


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["small", "small_edges", "served"])
def test_predict_scene_equals_predict_on_both_paths(which, served):
    model = served["small"] if which == "served" else fitted(which)
    be = model._backend()
    rows, (h, w) = S.load_scene_rows(FC.CASES["small"][0])
    want = model.predict(rows).astype(np.uint8).reshape(h, w)
    arrays, _ = FC.scene_arrays("small", be)
    for direct in (True, False, None):
        raster = torch.zeros(h * w, dtype=torch.uint8)
        model.predict_scene(arrays, raster, w, direct=direct)
        assert np.array_equal(raster.numpy().reshape(h, w), want), direct
    assert len(np.unique(want)) > 1


def test_chunked_serving_equals_one_launch():
    """chunk_rows cuts predict, predict_proba and the gather path of predict_scene into several launches that write at
    offsets into the same outputs."""
    model = fitted("small")
    _, _, Xv, _ = FC.load("small")
    rows, (h, w) = S.load_scene_rows(FC.CASES["small"][0])
    arrays, _ = FC.scene_arrays("small", model._backend())
    want = model.predict(rows), model.predict_proba(Xv)
    assert model.chunk_rows is None and model._chunk(10 ** 9) == (1 << 28) // (4 * 225)
    try:
        model.chunk_rows = 7  # 480 = 68 x 7 + 4, 24 = 3 x 7 + 3
        assert np.array_equal(model.predict(rows), want[0]) and np.array_equal(model.predict_proba(Xv), want[1])
        raster = torch.zeros(h * w, dtype=torch.uint8)
        model.predict_scene(arrays, raster, w, direct=False)
        assert np.array_equal(raster.numpy(), want[0].astype(np.uint8))
    finally:
        model.chunk_rows = None


def test_predict_scene_takes_the_gather_path_for_the_half_resolution_layout():
    """GRSS2018's layout (HSI at half the LiDAR resolution) is not what the direct kernel reads: gather + row kernel."""
    from hypelcnn_amd.common.common_nn_ops import SceneArrays, get_loader_from_name
    model = fitted("small")  # 5 x 5 x (8 + 1) features, as this scene's patches
    be = model._backend()
    ds = get_loader_from_name("SyntheticDataLoader", "grss2018hr:bands=8:classes=4:h=20:w=24").load_data(2, False)
    h, w = ds.get_scene_shape()[:2]
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    arrays = SceneArrays()
    arrays.feed(ds, np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(xs.size, dtype=int)], axis=1), be)
    assert arrays.casi_scale == 2
    rows = np.stack([ds.get_data_point(x, y).reshape(-1) for y in range(h) for x in range(w)]).astype(np.float32)
    raster = torch.zeros(h * w, dtype=torch.uint8)
    model.predict_scene(arrays, raster, w)
    assert np.array_equal(raster.numpy(), model.predict(rows).astype(np.uint8))
    with pytest.raises(ValueError, match="single-resolution"):
        model.predict_scene(arrays, raster, w, direct=True)


# 8 ---------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end_and_refusals(tmp_path):
    path = S.CASES["small_rbf"]["path"]
    common = ["--loader_name", "SyntheticDataLoader", "--path", path, "--neighborhood", "2"]
    out = T.main(["--estimator", "forest", "--forest_trees", "8", "--fullscene", "--base_log_path", str(tmp_path / "log"),
                  "--output_path", str(tmp_path / "out")] + common, backend=EmuBackend())
    est, predicted, cm, (oa, _, _), scene = out[0]
    assert isinstance(est, P.ForestClassifier) and est.n_estimators == 8 and est.seed == 0
    assert np.array_equal(est.arrays()["feature"], fitted("small").arrays()["feature"])  # the CLI's defaults = the case
    for name in ("confusion_matrix_SyntheticDataLoader_run0.csv", "metrics_SyntheticDataLoader_run0.txt",
                 "params_SyntheticDataLoader_run0.json"):
        assert os.path.getsize(tmp_path / "log" / name) > 0
    with open(tmp_path / "log" / "params_SyntheticDataLoader_run0.json") as f:
        assert json.load(f) == est.get_params()
    for name in ("result_raw.tif", "result_colorized.tif"):
        assert os.path.getsize(tmp_path / "out" / name) > 0
    rows, (h, w) = S.load_scene_rows("small_rbf")
    assert np.array_equal(scene, est.predict(rows).reshape(h, w)) and oa == np.trace(cm) / cm.sum()
    flags, _ = T.build_parser().parse_known_args([])
    assert (flags.forest_trees, flags.forest_max_features, flags.forest_bins, flags.forest_seed) == (50, 24, 256, 0)
    assert "forest" in T.ESTIMATORS and T.create_estimator(T.build_parser().parse_known_args(
        ["--estimator", "forest", "--forest_seed", "3"])[0], EmuBackend(), run_index=2).seed == 5
    for name in ("RandomForestClassifier", "random_forest", "rf", "ExtraTreesClassifier"):
        with pytest.raises(NotImplementedError, match="RandomForestClassifier.*--estimator forest"):
            T.main(["--estimator", name] + common, backend=EmuBackend())
    with pytest.raises(ValueError, match="svc_grid"):
        T.main(["--estimator", "forest", "--svc_grid"] + common, backend=EmuBackend())
    with pytest.raises(ValueError, match="at most 255 classes"):
        P.ForestClassifier(backend=EmuBackend()).fit(np.zeros((300, 2), np.float32), np.arange(300))
    with pytest.raises(ValueError, match="HYPEL_FOREST_MAX_CLASSES"):
        P.ForestClassifier(backend=EmuBackend()).fit(np.zeros((40, 2), np.float32), np.arange(40))
    m = P.ForestClassifier(n_estimators=1, backend=EmuBackend()).fit(np.arange(8, dtype=np.float32).reshape(4, 2),
                                                                      np.array([.5, .5, 1.5, 1.5]))
    with pytest.raises(ValueError, match="integers in 0..255"):
        m.predict_scene(None, None, 1)
    assert P.ForestClassifier(max_features="sqrt")._resolve_max_features(144) == 12
    assert P.ForestClassifier(max_features=None)._resolve_max_features(144) == 144
