"""TEST INFRASTRUCTURE: numpy twin of the random-forest entry points (include/hypel.h, hypel_forest_*), attached to
tests/emu_backend.EmuBackend on import.  Written from the header: integer histograms and int64 sums of squares are
exact, the score is two float64 divisions and one addition (numpy rounds each once, as the device must), choices among
equals follow the header's order (score, column, bin)."""
import numpy as np

from hypelcnn_amd.backend import (FOREST_EDGE_ROWS, FOREST_MAX_CLASSES, FOREST_MAX_DEPTH, FOREST_MAX_EDGES,
                                  FOREST_NODE_DTYPE)
from tests.emu_backend import EmuBackend, _arr, _mat
from tests.emu_scene import _typed

E = FOREST_MAX_EDGES


def column_edges(values, n_bins):
    """edges of one column from its sampled values (any order)"""
    s = np.sort(np.asarray(values, np.float32) + np.float32(0))
    n = len(s)
    out = []
    for j in range(1, n_bins):
        v = s[j * n // n_bins]
        if v >= s[-1]:
            break
        if not out or v != out[-1]:
            out.append(v)
    return np.array(out, np.float32)


def _k_forest_bin_edges_f32(self, x, ld, n, f, perm, n_bins, edges, n_edges):
    assert n > 0 and 0 < f <= ld and 2 <= n_bins <= E + 1
    n_s = min(n, FOREST_EDGE_ROWS)
    rows = _typed(perm, np.int32, n_s)
    assert len(np.unique(rows)) == n_s and rows.min() >= 0 and rows.max() < n
    m = _mat(x, ld, n, f)[rows]
    e = _typed(edges, np.float32, f * E).reshape(f, E)
    ne = _typed(n_edges, np.int32, f)
    e[...] = np.inf
    for c in range(f):
        got = column_edges(m[:, c], n_bins)
        e[c, :len(got)] = got
        ne[c] = len(got)


def _k_forest_bin_u8(self, x, ld, n, f, edges, n_edges, bins, ldn):
    assert n > 0 and 0 < f <= ld and ldn >= n
    m = _mat(x, ld, n, f)
    e = _typed(edges, np.float32, f * E).reshape(f, E)
    ne = _typed(n_edges, np.int32, f)
    b = _typed(bins, np.uint8, f * ldn).reshape(f, ldn)
    for c in range(f):
        b[c, :n] = np.searchsorted(e[c, :ne[c]], m[:, c], side="left")  # the number of edges < x


def node_histogram(bins_col, y, w, rows, n_classes):
    h = np.zeros((E + 1, n_classes), np.int64)
    np.add.at(h, (bins_col[rows], y[rows]), w[rows])
    return h


def best_boundary(h):
    """(score, bin, valid) of one histogram [256][classes]"""
    left = np.cumsum(h, 0)[:E]
    right = h.sum(0)[None, :] - left
    nl, nr = left.sum(1), right.sum(1)
    ok = (nl > 0) & (nr > 0)
    if not ok.any():
        return 0.0, -1, 0
    sl, sr = (left * left).sum(1), (right * right).sum(1)
    sc = np.full(E, -1.0)
    sc[ok] = sl[ok].astype(np.float64) / nl[ok].astype(np.float64) + sr[ok].astype(np.float64) / nr[ok].astype(np.float64)
    t = int(np.argmax(sc))  # the first maximum = the lowest bin
    return float(sc[t]), t, 1


def _k_forest_split_hist(self, bins, ldn, y, weight, n, n_classes, order, active, n_active, cand, max_features, f, score,
                         best_bin, valid):
    assert 1 <= n_classes <= FOREST_MAX_CLASSES and 1 <= max_features <= f and n_active > 0 and ldn >= n
    b = _typed(bins, np.uint8, f * ldn).reshape(f, ldn)
    yv, od = _typed(y, np.int32, n), _arr(order, np.int32)
    act = _typed(active, np.int32, 4 * n_active).reshape(n_active, 4)
    cd = _typed(cand, np.int32, n_active * max_features).reshape(n_active, max_features)
    wv = _arr(weight, np.int32)
    sc, bb, vd = (_typed(score, np.float64, cd.size), _typed(best_bin, np.int32, cd.size), _typed(valid, np.int32, cd.size))
    for a, (tree, start, count, _) in enumerate(act):
        assert len(set(cd[a])) == max_features and cd[a].min() >= 0 and cd[a].max() < f
        rows = od[start:start + count]
        w = wv[tree * n:(tree + 1) * n]
        for s, c in enumerate(cd[a]):
            at = a * max_features + s
            sc[at], bb[at], vd[at] = (0.0, -1, 0) if count < 2 else best_boundary(node_histogram(b[c], yv, w, rows, n_classes))


def _k_forest_split_apply(self, bins, ldn, y, weight, n, n_classes, order_in, order_out, active, n_active, cand,
                          max_features, f, score, best_bin, valid, edges, level, max_depth, node_base, node_capacity,
                          feature, thr_bin, threshold, left, right, node_tree, node_count, node_weight, value, split_ws,
                          next_active, counter):
    assert 1 <= n_classes <= FOREST_MAX_CLASSES and 1 <= max_features <= f and n_active > 0 and ldn >= n
    assert 0 <= max_depth <= FOREST_MAX_DEPTH and level >= 0 and 0 <= node_base <= node_capacity
    assert order_in.ptr() != order_out.ptr()
    b = _typed(bins, np.uint8, f * ldn).reshape(f, ldn)
    yv, src, dst = _typed(y, np.int32, n), _arr(order_in, np.int32), _arr(order_out, np.int32)
    act = _typed(active, np.int32, 4 * n_active).reshape(n_active, 4)
    shape = (n_active, max_features)
    cd = _typed(cand, np.int32, n_active * max_features).reshape(shape)
    sc = _typed(score, np.float64, cd.size).reshape(shape)
    bb, vd = _typed(best_bin, np.int32, cd.size).reshape(shape), _typed(valid, np.int32, cd.size).reshape(shape)
    e = _typed(edges, np.float32, f * E).reshape(f, E)
    wv = _arr(weight, np.int32)
    out = {k: _arr(r, np.int32) for k, r in (("feature", feature), ("thr_bin", thr_bin), ("left", left), ("right", right),
                                              ("tree", node_tree), ("count", node_count), ("weight", node_weight))}
    thr, val = _arr(threshold, np.float32), _arr(value, np.float64)
    ws = _typed(split_ws, np.int32, n_active)
    nxt = _typed(next_active, np.int32, 8 * n_active).reshape(2 * n_active, 4)
    r, overflow = 0, False
    for a, (tree, start, count, node) in enumerate(act):
        rows = src[start:start + count]
        w = wv[tree * n:(tree + 1) * n]
        cls = np.bincount(yv[rows], weights=None, minlength=n_classes) * 0
        np.add.at(cls, yv[rows], w[rows])
        nw = int(cls.sum())
        slots = [s for s in range(max_features) if vd[a, s]]
        leaf = count < 2 or (cls > 0).sum() < 2 or not slots or level >= max_depth
        out["tree"][node], out["count"][node], out["weight"][node] = tree, count, nw
        val[node * n_classes:(node + 1) * n_classes] = cls.astype(np.float64) / np.float64(nw)
        out["left"][node] = out["right"][node] = -1
        if leaf:
            out["feature"][node] = out["thr_bin"][node] = -1
            thr[node] = 0.0
            ws[a] = 0
            continue
        s = min(slots, key=lambda k: (-sc[a, k], cd[a, k], bb[a, k]))
        c, t = int(cd[a, s]), int(bb[a, s])
        out["feature"][node], out["thr_bin"][node], thr[node] = c, t, e[c, t]
        go_left = b[c][rows] <= t
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


def forest_means(read, tree_off, feature, threshold, left, right, leaf, leaf_value, n_rows):
    """mean leaf row per row; read(rows, node feature codes) -> float32 values"""
    n_trees, n_cls = len(tree_off), leaf_value.shape[1]
    total = np.zeros((n_rows, n_cls), np.float64)
    rows = np.arange(n_rows)
    for t in range(n_trees):
        node = np.full(n_rows, tree_off[t], np.int64)
        while True:
            inner = leaf[node] < 0
            if not inner.any():
                break
            at = node[inner]
            v = read(rows[inner], feature[at])
            node[inner] = np.where(v <= threshold[at], left[at], right[at])
        total += leaf_value[leaf[node]]  # tree order, one fp64 addition per tree and class
    return total / np.float64(n_trees)


def _model(tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes):
    assert n_trees > 0 and n_nodes >= n_trees and 0 < n_leaves <= n_nodes and 1 <= n_classes <= FOREST_MAX_CLASSES
    assert nodes.ptr() % FOREST_NODE_DTYPE.itemsize == 0
    rec = _typed(nodes, np.uint8, n_nodes * FOREST_NODE_DTYPE.itemsize).view(FOREST_NODE_DTYPE)
    l, r = rec["left"], rec["right"]
    lf = np.where(l < 0, -1 - l, -1)
    inner = lf < 0
    assert (l[inner] > np.flatnonzero(inner)).all() and (r[inner] > np.flatnonzero(inner)).all()
    assert l[inner].max(initial=0) < n_nodes and r[inner].max(initial=0) < n_nodes and lf.max() < n_leaves
    return (_typed(tree_off, np.int32, n_trees), rec["feature"], rec["threshold"], l, r, lf,
            _typed(leaf_value, np.float64, n_leaves * n_classes).reshape(n_leaves, n_classes))


def _write_labels(win, class_labels, points, out, raster_w, n):
    lab = win.astype(np.uint8) if class_labels is None else _arr(class_labels, np.uint8)[win]
    o = _arr(out, np.uint8)
    if points is None:
        o[:n] = lab
    else:
        pts = _typed(points, np.int32, 2 * n).reshape(n, 2)
        o[pts[:, 1].astype(np.int64) * raster_w + pts[:, 0]] = lab


def _k_forest_predict_rows(self, x, ld, n, f, tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes,
                           class_labels, points, out, raster_w, proba):
    assert n > 0 and 0 < f <= ld
    model = _model(tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes)
    assert model[1].min() >= 0 and model[1].max() < f
    m = _mat(x, ld, n, f)
    mean = forest_means(lambda rows, feat: m[rows, feat], *model, n)
    if proba is not None:
        _typed(proba, np.float64, n * n_classes)[:] = mean.reshape(-1)
    _write_labels(np.argmax(mean, 1), class_labels, points, out, raster_w, n)


def _k_forest_predict_scene(self, casi, lidar, hp, wp, cc, cl, points, n, p, tree_off, n_trees, scene_nodes, n_nodes,
                            leaf_value, n_leaves, n_classes, class_labels, out, raster_w):
    assert n > 0 and p > 0 and hp >= p and wp >= p and cc > 0 and cl >= 0 and (cl == 0 or lidar is not None)
    model = _model(tree_off, n_trees, scene_nodes, n_nodes, leaf_value, n_leaves, n_classes)
    cs = _typed(casi, np.float32, hp * wp * cc)
    ls = None if cl == 0 else _typed(lidar, np.float32, hp * wp * cl)
    pts = _typed(points, np.int32, 2 * n).reshape(n, 2).astype(np.int64)
    assert (pts >= 0).all() and (pts[:, 0] + p <= wp).all() and (pts[:, 1] + p <= hp).all()
    origin = pts[:, 1] * wp + pts[:, 0]

    def read(rows, code):
        e, which = code >> 1, code & 1
        v = cs[np.where(which == 0, origin[rows] * cc + e, 0)]
        if ls is not None:
            v = np.where(which == 1, ls[np.where(which == 1, origin[rows] * cl + e, 0)], v)
        return v

    mean = forest_means(read, *model, n)
    _write_labels(np.argmax(mean, 1), class_labels, points, out, raster_w, n)


for _name, _fn in list(globals().items()):
    if _name.startswith("_k_forest_"):
        setattr(EmuBackend, _name[1:], _fn)
