"""TEST INFRASTRUCTURE shared by tests/golden/make_reference_forest.py and the forest tests: the cases, their inputs
(re-made from SyntheticDataLoader through tests/svm_cases.load_case_data, never stored) and the checks that run
unchanged on the emulation and on the device."""
import json
import os

import numpy as np

from tests import svm_cases as S

JSON_PATH = os.path.join(S.GOLDEN, "reference_forest.json")
NPZ_PATH = os.path.join(S.GOLDEN, "reference_forest.npz")

# case -> (the svm case whose scene it shares, ForestClassifier arguments)
CASES = {
    "small": ("small_rbf", dict(n_estimators=8, max_features=24)),        # N=215, F=225, 4 classes
    "small_edges": ("small_rbf", dict(n_estimators=8, max_features=300)),  # planted columns, two classes, clamped
    "grss2013": ("grss2013_rbf", dict(n_estimators=8, max_features=24)),  # N=2159, F=3625, 15 classes
}
CONSTANT_COL, THREE_COL, TIE_LOW, TIE_HIGH = 3, 5, 20, 120
TIE_EPS = 1e-12   # a row is left out when its two largest fixture probabilities are this close
SK_TREES = 50


def _plant(X, y2):
    X = X.copy()
    X[:, CONSTANT_COL] = 7.0
    X[:, THREE_COL] = np.float32(np.digitize(X[:, THREE_COL], np.quantile(X[:, THREE_COL], [1 / 3, 2 / 3])))
    # a strong but imperfect column, twice: the exact score tie must go to the lower index
    noise = np.random.Generator(np.random.PCG64(1234)).random(len(X)) * 1.3
    X[:, TIE_LOW] = X[:, TIE_HIGH] = (y2 + noise).astype(np.float32)
    return X


_cache = {}


def load(case):
    """(X_train, y_train, X_val, y_val) float32 / integer labels"""
    if case not in _cache:
        X, y, Xv, yv, _ = S.load_case_data(CASES[case][0])
        if case == "small_edges":
            cls = np.unique(y)
            y, yv = np.searchsorted(cls, y) // 2, np.searchsorted(cls, yv) // 2
            X, Xv = _plant(X, y), _plant(Xv, yv)
        _cache[case] = (X, np.asarray(y), Xv, np.asarray(yv))
    return _cache[case]


def recording_forest():
    """ForestClassifier that keeps, for the first `record_levels` levels of a fit, the level's tables in level_records_
    -- (active records, cand, score, bin, valid) -- and the device-to-model node map in model_node_."""
    from hypelcnn_amd.classic.forest import ForestClassifier

    class RecordingForest(ForestClassifier):
        record_levels = 0

        def fit(self, X, y):
            self.level_records_ = []
            return super().fit(X, y)

        def _level_done(self, level, active, n_active, cand, score, best_bin, valid):
            if level < self.record_levels:
                self.level_records_.append((active.cpu().numpy()[:4 * n_active].reshape(n_active, 4).copy(), cand,
                                            score.cpu().numpy().copy(), best_bin.cpu().numpy().copy(),
                                            valid.cpu().numpy().copy()))

        def _nodes_renumbered(self, model_node):
            self.model_node_ = model_node

    return RecordingForest


def make(case, backend, **override):
    args = dict(CASES[case][1])
    args.update(override)
    return recording_forest()(backend=backend, **args)


# the single-tree fixture's scene: `small` with another seed and six classes.  On `small` itself scikit-learn's own
# random_state changes the tree below the root (several columns split equally well there); on this scene its
# random_states 0, 1, 2 give one tree down to its last leaf (tests/golden/make_reference_forest.py asserts it)
TREE_PATH = "grss2013:bands=8:classes=6:h=20:w=24:seed=2"


def load_tree_case():
    """(X_train, y_train) of the single-tree fixture"""
    if "tree" not in _cache:
        from hypelcnn_amd.importer.InMemoryImporter import InMemoryImporter
        tr = InMemoryImporter().read_data_set("SyntheticDataLoader", TREE_PATH, 0.1, 0, S.NEIGHBORHOOD, False)[0]
        _cache["tree"] = (tr.data.reshape(len(tr.data), -1), np.asarray(tr.labels))
    return _cache["tree"]


def load_fixture():
    with open(JSON_PATH) as f:
        meta = json.load(f)
    return meta, np.load(NPZ_PATH)


def sk_arrays(fx, case):
    """from_arrays arguments of the stored scikit-learn forest"""
    k = f"{case}/rf/"
    return dict(classes=fx[k + "classes"], n_features=int(fx[k + "n_features"]), feature=fx[k + "feature"],
                threshold=fx[k + "threshold"], left=fx[k + "left"], right=fx[k + "right"],
                tree_offsets=fx[k + "tree_offsets"], value=leaf_rows_to_value(fx[k + "leaf_nodes"], fx[k + "leaf_rows"],
                                                                               len(fx[k + "feature"])))


def leaf_rows_to_value(leaf_nodes, leaf_rows, n_nodes):
    value = np.zeros((n_nodes, leaf_rows.shape[1]), np.float64)
    value[leaf_nodes] = leaf_rows
    return value


def left_out(proba):
    top = np.sort(proba, 1)
    return top[:, -1] - top[:, -2] <= TIE_EPS


def check_served_labels(pred, proba_ref, labels_ref, what):
    """The fixture's labels exactly, except rows whose two largest fixture probabilities are within TIE_EPS (<= 1 %)."""
    out = left_out(proba_ref)
    wrong = (np.asarray(pred).reshape(-1) != labels_ref) & ~out
    print(f"{what}: {int(wrong.sum())} rows differ, {int(out.sum())} of {len(labels_ref)} left out")
    assert out.mean() <= 0.01
    assert not wrong.any()


def scene_arrays(case, backend):
    """(SceneArrays over every pixel of the case's scene, (h, w))"""
    from hypelcnn_amd.common.common_nn_ops import SceneArrays, get_loader_from_name
    ds = get_loader_from_name("SyntheticDataLoader", S.CASES[CASES[case][0]]["path"]).load_data(S.NEIGHBORHOOD, False)
    h, w = ds.get_scene_shape()[:2]
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    targets = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(xs.size, dtype=int)], axis=1)
    arrays = SceneArrays()
    arrays.feed(ds, targets, backend)
    return arrays, (h, w)
