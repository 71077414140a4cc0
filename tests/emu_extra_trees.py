"""TEST INFRASTRUCTURE: numpy twin of the extra-trees entry points (include/hypel.h, hypel_forest_columns_f32,
hypel_forest_split_random, hypel_forest_split_apply_thr), attached to tests/emu_backend.EmuBackend on import like
tests/emu_forest.py.  Written from the header: the cut is three float32 numpy operations (one rounding each) and the
fallback; class weights and sums of squares are exact integers; the score is two float64 divisions and one addition;
the choice among equals is (score, column)."""
import numpy as np

from hypelcnn_amd.backend import FOREST_MAX_CLASSES, FOREST_MAX_DEPTH
from tests.emu_backend import EmuBackend, _arr, _mat
from tests.emu_scene import _typed


def _k_forest_columns_f32(self, x, ld, n, f, xt, ldn):
    assert n > 0 and 0 < f <= ld and ldn >= n
    out = _typed(xt, np.float32, f * ldn).reshape(f, ldn)
    out[:, :n] = _mat(x, ld, n, f).T + np.float32(0)


def random_cut(lo, hi, u):
    """the cut of one record from float32 lo < hi and u"""
    with np.errstate(over="ignore", invalid="ignore"):  # (hi - lo may be inf, 0 * inf a NaN)
        t = np.float32(lo + np.float32(u * np.float32(hi - lo)))
    if not (t < hi):
        t = lo
    return t


def cut_score(go_left, y, w, n_classes):
    left = np.bincount(y[go_left], w[go_left], n_classes).astype(np.int64)
    right = np.bincount(y[~go_left], w[~go_left], n_classes).astype(np.int64)
    return (np.float64((left * left).sum()) / np.float64(left.sum()) +
            np.float64((right * right).sum()) / np.float64(right.sum()))


def _k_forest_split_random(self, xt, ldn, y, weight, n, n_classes, order, active, n_active, cand, u, max_features, f,
                           score, thr, valid):
    assert 1 <= n_classes <= FOREST_MAX_CLASSES and 1 <= max_features <= f and n_active > 0 and ldn >= n
    cols = _typed(xt, np.float32, f * ldn).reshape(f, ldn)
    yv, od, wv = _typed(y, np.int32, n), _arr(order, np.int32), _arr(weight, np.int32)
    act = _typed(active, np.int32, 4 * n_active).reshape(n_active, 4)
    cd = _typed(cand, np.int32, n_active * max_features).reshape(n_active, max_features)
    uv = _typed(u, np.float32, cd.size)
    sc, th, vd = _typed(score, np.float64, cd.size), _typed(thr, np.float32, cd.size), _typed(valid, np.int32, cd.size)
    for a, (tree, start, count, _) in enumerate(act):
        assert len(set(cd[a])) == max_features and cd[a].min() >= 0 and cd[a].max() < f
        rows = od[start:start + count]
        w = wv[tree * n:(tree + 1) * n][rows].astype(np.int64)
        for s, c in enumerate(cd[a]):
            at = a * max_features + s
            v = cols[c][rows]
            sc[at], th[at], vd[at] = 0.0, 0.0, 0
            if count < 2 or not v.min() < v.max():
                continue
            t = random_cut(v.min(), v.max(), uv[at])
            sc[at], th[at], vd[at] = cut_score(v <= t, yv[rows], w, n_classes), t, 1


def _k_forest_split_apply_thr(self, xt, ldn, y, weight, n, n_classes, order_in, order_out, active, n_active, cand,
                              max_features, f, score, thr, valid, level, max_depth, node_base, node_capacity, feature,
                              thr_bin, threshold, left, right, node_tree, node_count, node_weight, value, split_ws,
                              next_active, counter):
    assert 1 <= n_classes <= FOREST_MAX_CLASSES and 1 <= max_features <= f and n_active > 0 and ldn >= n
    assert 0 <= max_depth <= FOREST_MAX_DEPTH and level >= 0 and 0 <= node_base <= node_capacity
    assert order_in.ptr() != order_out.ptr()
    cols = _typed(xt, np.float32, f * ldn).reshape(f, ldn)
    yv, src, dst = _typed(y, np.int32, n), _arr(order_in, np.int32), _arr(order_out, np.int32)
    act = _typed(active, np.int32, 4 * n_active).reshape(n_active, 4)
    shape = (n_active, max_features)
    cd = _typed(cand, np.int32, n_active * max_features).reshape(shape)
    sc = _typed(score, np.float64, cd.size).reshape(shape)
    th, vd = _typed(thr, np.float32, cd.size).reshape(shape), _typed(valid, np.int32, cd.size).reshape(shape)
    wv = _arr(weight, np.int32)
    out = {k: _arr(r, np.int32) for k, r in (("feature", feature), ("thr_bin", thr_bin), ("left", left), ("right", right),
                                              ("tree", node_tree), ("count", node_count), ("weight", node_weight))}
    tv, val = _arr(threshold, np.float32), _arr(value, np.float64)
    ws = _typed(split_ws, np.int32, n_active)
    nxt = _typed(next_active, np.int32, 8 * n_active).reshape(2 * n_active, 4)
    r, overflow = 0, False
    for a, (tree, start, count, node) in enumerate(act):
        rows = src[start:start + count]
        cls = np.bincount(yv[rows], wv[tree * n:(tree + 1) * n][rows], n_classes).astype(np.int64)
        nw = int(cls.sum())
        slots = [s for s in range(max_features) if vd[a, s]]
        leaf = count < 2 or (cls > 0).sum() < 2 or not slots or level >= max_depth
        out["tree"][node], out["count"][node], out["weight"][node] = tree, count, nw
        val[node * n_classes:(node + 1) * n_classes] = cls.astype(np.float64) / np.float64(nw)
        out["left"][node] = out["right"][node] = out["thr_bin"][node] = -1
        if leaf:
            out["feature"][node], tv[node], ws[a] = -1, 0.0, 0
            continue
        s = min(slots, key=lambda k: (-sc[a, k], cd[a, k]))
        c, t = int(cd[a, s]), th[a, s]
        out["feature"][node], tv[node] = c, t
        go_left = cols[c][rows] <= t
        n_left = int(go_left.sum())
        dst[start:start + count] = np.concatenate([rows[go_left], rows[~go_left]])
        ws[a] = n_left
        lid = node_base + 2 * r
        if lid + 1 < node_capacity:
            out["left"][node], out["right"][node] = lid, lid + 1
            nxt[2 * r] = (tree, start, n_left, lid)
            nxt[2 * r + 1] = (tree, start + n_left, count - n_left, lid + 1)
        else:
            overflow = True
        r += 1
    _arr(counter, np.int32)[0] = -1 if overflow else 2 * r


for _name, _fn in list(globals().items()):
    if _name.startswith("_k_forest_"):
        setattr(EmuBackend, _name[1:], _fn)
