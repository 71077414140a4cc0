"""TEST INFRASTRUCTURE shared by tests/test_extra_trees_emu.py and tests/test_gpu_extra_trees.py: a recording
ExtraTreesForest, the scikit-learn fixture of tests/golden/make_reference_extra_trees.py, and a brute-force fit that
replays the draw order ExtraTreesForest documents -- node by node in plain numpy and Python ints, written from the class
docstring and include/hypel.h, sharing no code with the class, the kernels or tests/emu_forest.py."""
import numpy as np

from hypelcnn_amd.backend import FOREST_MAX_DEPTH
from tests.golden.make_reference_extra_trees import PATH as NPZ_PATH

F32 = np.float32


def recording_extra_trees():
    """ExtraTreesForest that keeps every level's tables in level_records_: (active records, cand, score, thr, valid)"""
    from hypelcnn_amd.classic.forest import ExtraTreesForest

    class RecordingExtraTrees(ExtraTreesForest):
        def fit(self, X, y):
            self.level_records_ = []
            return super().fit(X, y)

        def _level_done(self, level, active, n_active, cand, score, thr, valid):
            self.level_records_.append((active.cpu().numpy()[:4 * n_active].reshape(n_active, 4).copy(), cand,
                                        score.cpu().numpy().copy(), thr.cpu().numpy().copy(), valid.cpu().numpy().copy()))

    return RecordingExtraTrees


_fixture = {}


def load_fixture():
    if not _fixture:
        _fixture.update(np.load(NPZ_PATH))
    return _fixture


def brute_fit(X, y, n_estimators, max_features, seed, bootstrap=False, max_depth=None):
    """(arrays() of the fitted model, n_levels_) by the documented rules: the bootstrap counts if asked for; per level
    the candidate table (one rng.choice per active node unless every column is a candidate), then u; per node and slot
    lo, hi, the float32 cut with its fallback, the integer class weights of both sides, the score; the largest score,
    then the lower column; children numbered in active-node order."""
    X = np.asarray(X, F32) + F32(0)
    classes, yi = np.unique(np.asarray(y), return_inverse=True)
    n, f = X.shape
    C, mf = len(classes), min(int(max_features), f)
    rng = np.random.Generator(np.random.PCG64(seed))
    if bootstrap:
        weight = [np.bincount(rng.integers(0, n, n), minlength=n) for _ in range(n_estimators)]
    else:
        weight = [np.ones(n, np.int64) for _ in range(n_estimators)]
    cap = FOREST_MAX_DEPTH if max_depth is None else max_depth
    nodes = [dict(tree=t, rows=np.flatnonzero(weight[t] > 0)) for t in range(n_estimators)]
    active, level = list(range(n_estimators)), 0
    while active and level <= cap:
        if mf == f:
            cand = [list(range(f))] * len(active)
        else:
            cand = [rng.choice(f, mf, replace=False) for _ in active]
        u = rng.random((len(active), mf), dtype=F32)
        nxt = []
        for a, at in enumerate(active):
            nd = nodes[at]
            rows = nd["rows"]
            w = [int(v) for v in weight[nd["tree"]][rows]]
            cls = [0] * C
            for k, v in zip(yi[rows], w):
                cls[k] += v
            best = None
            for s, c in enumerate(cand[a]):
                vals = X[rows, c]
                lo, hi = vals.min(), vals.max()
                if len(rows) < 2 or not lo < hi:
                    continue
                with np.errstate(over="ignore", invalid="ignore"):
                    t = F32(lo + F32(u[a, s] * F32(hi - lo)))
                if not t < hi:
                    t = lo
                left, right = [0] * C, [0] * C
                for k, v, x in zip(yi[rows], w, vals):
                    (left if x <= t else right)[k] += v
                score = float(sum(v * v for v in left)) / float(sum(left)) + \
                    float(sum(v * v for v in right)) / float(sum(right))
                if best is None or (-score, int(c)) < best[0]:
                    best = ((-score, int(c)), t)
            nd["value"] = [float(v) / float(sum(cls)) for v in cls]
            nd["feature"], nd["threshold"], nd["left"], nd["right"] = -1, F32(0), -1, -1
            if len(rows) < 2 or sum(1 for v in cls if v > 0) < 2 or best is None or level >= cap:
                continue
            (_, c), t = best
            go = X[rows, c] <= t
            nd["feature"], nd["threshold"], nd["left"], nd["right"] = c, t, len(nodes), len(nodes) + 1
            nodes += [dict(tree=nd["tree"], rows=rows[go]), dict(tree=nd["tree"], rows=rows[~go])]
            nxt += [nd["left"], nd["right"]]
        active, level = nxt, level + 1
    by_tree = sorted(range(len(nodes)), key=lambda k: nodes[k]["tree"])  # (stable: breadth-first inside a tree)
    place = {k: at for at, k in enumerate(by_tree)}
    offsets = np.concatenate([[0], np.cumsum(np.bincount([nd["tree"] for nd in nodes], minlength=n_estimators))])
    local = lambda k, key: -1 if nodes[k][key] < 0 else place[nodes[k][key]] - offsets[nodes[k]["tree"]]  # noqa: E731
    return {"feature": np.array([nodes[k]["feature"] for k in by_tree], np.int32),
            "threshold": np.array([nodes[k]["threshold"] for k in by_tree], F32),
            "left": np.array([local(k, "left") for k in by_tree], np.int32),
            "right": np.array([local(k, "right") for k in by_tree], np.int32),
            "tree_offsets": offsets.astype(np.int32),
            "value": np.array([nodes[k]["value"] for k in by_tree], np.float64)}, level


def same_arrays(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)
