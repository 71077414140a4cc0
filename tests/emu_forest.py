"""TEST INFRASTRUCTURE: numpy twin of the forest family's entry points (include/hypel.h, hypel_forest_*: the histogram
forest, extra-trees and the diagnostics), attached to tests/emu_backend.EmuBackend on import.  Written from the header:
integer histograms, class weights and int64 sums of squares are exact, a score is two float64 divisions and one addition
(numpy rounds each once, as the device must), an extra-trees cut is three float32 operations and the fallback, choices
among equals follow the header's order (score, column, bin).  The votes are fp64 additions in tree order (a tree that
does not vote adds nothing, not a zero), every importance sum is a sequential np.add.accumulate / np.add.at -- numpy's
pairwise np.sum is never used where the header fixes an order.  Each algorithm is here once: _split_apply for both
searches, leaf_rows + vote for serving, out-of-bag and permuted hits."""
import inspect
import sys

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


def _k_forest_columns_f32(self, x, ld, n, f, xt, ldn):
    assert n > 0 and 0 < f <= ld and ldn >= n
    out = _typed(xt, np.float32, f * ldn).reshape(f, ldn)
    out[:, :n] = _mat(x, ld, n, f).T + np.float32(0)


# ---- the two split searches ------------------------------------------------------------------------------------------
def _level(y, weight, n, n_classes, order, active, n_active, cand, max_features, f, ldn, *records):
    """the operands every growth entry point reads, and its per-record tables as flat arrays of their dtype"""
    assert 1 <= n_classes <= FOREST_MAX_CLASSES and 1 <= max_features <= f and n_active > 0 and ldn >= n
    cd = _typed(cand, np.int32, n_active * max_features).reshape(n_active, max_features)
    return (_typed(y, np.int32, n), _arr(weight, np.int32), _arr(order, np.int32),
            _typed(active, np.int32, 4 * n_active).reshape(n_active, 4), cd,
            *[_typed(ref, dtype, cd.size) for ref, dtype in records])


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
    yv, wv, od, act, cd, sc, bb, vd = _level(y, weight, n, n_classes, order, active, n_active, cand, max_features, f, ldn,
                                             (score, np.float64), (best_bin, np.int32), (valid, np.int32))
    b = _typed(bins, np.uint8, f * ldn).reshape(f, ldn)
    for a, (tree, start, count, _) in enumerate(act):
        assert len(set(cd[a])) == max_features and cd[a].min() >= 0 and cd[a].max() < f
        rows = od[start:start + count]
        w = wv[tree * n:(tree + 1) * n]
        for s, c in enumerate(cd[a]):
            at = a * max_features + s
            sc[at], bb[at], vd[at] = (0.0, -1, 0) if count < 2 else best_boundary(node_histogram(b[c], yv, w, rows, n_classes))


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
    yv, wv, od, act, cd, uv, sc, th, vd = _level(y, weight, n, n_classes, order, active, n_active, cand, max_features, f,
                                                 ldn, (u, np.float32), (score, np.float64), (thr, np.float32),
                                                 (valid, np.int32))
    cols = _typed(xt, np.float32, f * ldn).reshape(f, ldn)
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


def _split_apply(table, cut, tie, ldn, y, weight, n, n_classes, order_in, order_out, active, n_active, cand, max_features,
                 f, score, valid, level, max_depth, node_base, node_capacity, feature, thr_bin, threshold, left, right,
                 node_tree, node_count, node_weight, value, split_ws, next_active, counter):
    """One level's apply for either search.  A row of column c goes left where table[c][row] <= the cut of the winning
    slot; cut[a, s] is that cut, tie(a, s) the keys that order slots of equal score and column (a tuple), and the
    caller writes thr_bin and threshold of the split nodes from the returned [(node, column, cut)]."""
    assert 0 <= max_depth <= FOREST_MAX_DEPTH and level >= 0 and 0 <= node_base <= node_capacity
    assert order_in.ptr() != order_out.ptr()
    yv, wv, src, act, cd, sc, vd = _level(y, weight, n, n_classes, order_in, active, n_active, cand, max_features, f, ldn,
                                          (score, np.float64), (valid, np.int32))
    sc, vd, dst = sc.reshape(cd.shape), vd.reshape(cd.shape), _arr(order_out, np.int32)
    out = {k: _arr(r, np.int32) for k, r in (("feature", feature), ("thr_bin", thr_bin), ("left", left), ("right", right),
                                              ("tree", node_tree), ("count", node_count), ("weight", node_weight))}
    thr, val = _arr(threshold, np.float32), _arr(value, np.float64)
    ws = _typed(split_ws, np.int32, n_active)
    nxt = _typed(next_active, np.int32, 8 * n_active).reshape(2 * n_active, 4)
    split, overflow = [], False
    for a, (tree, start, count, node) in enumerate(act):
        rows = src[start:start + count]
        cls = np.zeros(n_classes, np.int64)
        np.add.at(cls, yv[rows], wv[tree * n:(tree + 1) * n][rows])
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
        s = min(slots, key=lambda k: (-sc[a, k], cd[a, k]) + tie(a, k))
        c = out["feature"][node] = int(cd[a, s])
        go_left = table[c][rows] <= cut[a, s]
        n_left = int(go_left.sum())
        dst[start:start + count] = np.concatenate([rows[go_left], rows[~go_left]])
        ws[a] = n_left
        lid = node_base + 2 * len(split)
        if lid + 1 < node_capacity:
            out["left"][node], out["right"][node] = lid, lid + 1
            nxt[2 * len(split)] = (tree, start, n_left, lid)
            nxt[2 * len(split) + 1] = (tree, start + n_left, count - n_left, lid + 1)
        else:
            overflow = True
        split.append((node, c, cut[a, s]))
    _arr(counter, np.int32)[0] = -1 if overflow else 2 * len(split)
    return split, out["thr_bin"], thr


def _k_forest_split_apply(self, bins, ldn, y, weight, n, n_classes, order_in, order_out, active, n_active, cand,
                          max_features, f, score, best_bin, valid, edges, *grown):
    bb = _typed(best_bin, np.int32, n_active * max_features).reshape(n_active, max_features)
    e = _typed(edges, np.float32, f * E).reshape(f, E)
    split, thr_bin, threshold = _split_apply(_typed(bins, np.uint8, f * ldn).reshape(f, ldn), bb, lambda a, k: (bb[a, k],),
                                             ldn, y, weight, n, n_classes, order_in, order_out, active, n_active, cand,
                                             max_features, f, score, valid, *grown)
    for node, c, t in split:
        thr_bin[node], threshold[node] = t, e[c, t]


def _k_forest_split_apply_thr(self, xt, ldn, y, weight, n, n_classes, order_in, order_out, active, n_active, cand,
                              max_features, f, score, thr, valid, *grown):
    th = _typed(thr, np.float32, n_active * max_features).reshape(n_active, max_features)
    split, thr_bin, threshold = _split_apply(_typed(xt, np.float32, f * ldn).reshape(f, ldn), th, lambda a, k: (),
                                             ldn, y, weight, n, n_classes, order_in, order_out, active, n_active, cand,
                                             max_features, f, score, valid, *grown)
    for node, c, t in split:  # (a node's columns are distinct: the column decides every tie; no bin)
        thr_bin[node], threshold[node] = -1, t


# ---- the walk: serving, out-of-bag, permuted hits ----------------------------------------------------------------------
def _model(tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes):
    assert tree_off is not None and nodes is not None and leaf_value is not None
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


def leaf_rows(read, tree_off, feature, threshold, left, right, leaf, n_rows):
    """[n_trees][n_rows]: the leaf-table row every row ends in, tree by tree; read(rows, features) -> float32 values"""
    out = np.zeros((len(tree_off), n_rows), np.int64)
    rows = np.arange(n_rows)
    for t in range(len(tree_off)):
        node = np.full(n_rows, tree_off[t], np.int64)
        while True:
            inner = leaf[node] < 0
            if not inner.any():
                break
            at = node[inner]
            node[inner] = np.where(read(rows[inner], feature[at]) <= threshold[at], left[at], right[at])
        out[t] = leaf[node]
    return out


def vote(ends, leaf_value, voting=None):
    """(mean [n][C], votes [n], first maximum [n]) of the trees `voting` [n_trees][n] (bool; None: every tree), added in
    tree order, one fp64 addition per voting tree and class"""
    if voting is None:
        voting = np.ones(ends.shape, bool)
    total = np.zeros((ends.shape[1], leaf_value.shape[1]), np.float64)
    for t in range(ends.shape[0]):
        total[voting[t]] += leaf_value[ends[t][voting[t]]]
    votes = voting.sum(0).astype(np.int32)
    mean = np.zeros_like(total)
    np.divide(total, votes[:, None].astype(np.float64), out=mean, where=votes[:, None] > 0)
    return mean, votes, np.argmax(mean, 1)


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
    mean, _, win = vote(leaf_rows(lambda rows, feat: m[rows, feat], *model[:6], n), model[6])
    if proba is not None:
        _typed(proba, np.float64, n * n_classes)[:] = mean.reshape(-1)
    _write_labels(win, class_labels, points, out, raster_w, n)


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

    _write_labels(vote(leaf_rows(read, *model[:6], n), model[6])[2], class_labels, points, out, raster_w, n)


def _k_forest_oob_rows(self, x, ld, n, f, tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes,
                       class_labels, weight, ldw, out, proba, votes):
    assert n > 0 and 0 < f <= ld and ldw >= n
    assert x is not None and weight is not None and out is not None and proba is not None and votes is not None
    model = _model(tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes)
    m = _mat(x, ld, n, f)
    in_bag = _mat(weight, ldw, n_trees, n, np.int32)
    mean, nv, win = vote(leaf_rows(lambda rows, feat: m[rows, feat], *model[:6], n), model[6], ~(in_bag > 0))
    _typed(proba, np.float64, n * n_classes)[:] = mean.reshape(-1)
    _typed(votes, np.int32, n)[:] = nv
    _write_labels(win, class_labels, None, out, 0, n)


def _k_forest_permuted_hits(self, x, ld, n, f, tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes, y,
                            partner, n_repeats, group_mod, g0, n_groups, hits):
    assert n > 0 and 0 < f <= ld and n_repeats >= 1
    assert x is not None and y is not None and partner is not None and hits is not None
    assert group_mod >= 1 and g0 >= 0 and n_groups >= 1 and g0 + n_groups <= group_mod
    assert n_groups * n_repeats * ((n + 63) // 64) < 1 << 31
    model = _model(tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes)
    m = _mat(x, ld, n, f)
    yv = _typed(y, np.int32, n)
    pt = _typed(partner, np.int32, n_repeats * n).reshape(n_repeats, n)
    h = _typed(hits, np.int32, n_groups * n_repeats).reshape(n_groups, n_repeats)
    for g in range(g0, g0 + n_groups):
        cols = np.arange(f)[np.arange(f) % group_mod == g]
        for r in range(n_repeats):
            assert np.array_equal(np.sort(pt[r]), np.arange(n))
            mixed = m.copy()
            mixed[:, cols] = m[pt[r]][:, cols]
            ends = leaf_rows(lambda rows, feat: mixed[rows, feat], *model[:6], n)
            h[g - g0, r] += int((vote(ends, model[6])[2] == yv).sum())


# ---- mean decrease in impurity -----------------------------------------------------------------------------------------
def node_gini(value):
    s = np.zeros(value.shape[0], np.float64)
    for k in range(value.shape[1]):  # class order, product and addition rounded once each
        s = s + value[:, k] * value[:, k]
    return 1.0 - s


def ordered_sum(a):
    """the sum of a 1-d float64 array in ascending index order from 0.0"""
    return np.add.accumulate(np.concatenate([[0.0], a]))[-1]


def _k_forest_importances_f64(self, nodes, n_nodes, tree_off, n_trees, value, n_classes, node_weight, impurity, f,
                              per_tree, importances, n_used):
    assert n_trees > 0 and n_nodes >= n_trees and f > 0
    assert nodes is not None and tree_off is not None and nodes.ptr() % FOREST_NODE_DTYPE.itemsize == 0
    assert node_weight is not None and per_tree is not None and importances is not None and n_used is not None
    rec = _typed(nodes, np.uint8, n_nodes * FOREST_NODE_DTYPE.itemsize).view(FOREST_NODE_DTYPE)
    off = np.concatenate([_typed(tree_off, np.int32, n_trees), [n_nodes]]).astype(np.int64)
    w = _typed(node_weight, np.float64, n_nodes)
    if impurity is None:
        assert value is not None and 1 <= n_classes <= FOREST_MAX_CLASSES
        imp = node_gini(_typed(value, np.float64, n_nodes * n_classes).reshape(n_nodes, n_classes))
    else:
        imp = _typed(impurity, np.float64, n_nodes)
    pt = _typed(per_tree, np.float64, n_trees * f).reshape(n_trees, f)
    out = _typed(importances, np.float64, f)
    l, r = rec["left"].astype(np.int64), rec["right"].astype(np.int64)
    wi = w * imp
    total, used = np.zeros(f, np.float64), 0
    for t in range(n_trees):
        at = np.arange(off[t], off[t + 1])
        at = at[l[at] >= 0]
        raw = np.zeros(f, np.float64)
        np.add.at(raw, rec["feature"][at], (wi[at] - wi[l[at]]) - wi[r[at]])  # unbuffered: in the order of `at`
        raw = raw / w[off[t]]
        s = ordered_sum(raw)
        pt[t] = raw / s if s > 0 else raw
        if off[t + 1] - off[t] > 1:
            total = total + pt[t]
            used += 1
    mean = total / np.float64(used) if used else np.zeros(f)
    s = ordered_sum(mean)
    out[:] = mean / s if s > 0 else mean
    _arr(n_used, np.int32)[0] = used


for _name, _fn in list(globals().items()):
    if _name.startswith("_k_forest_"):
        setattr(EmuBackend, _name[1:], _fn)


def mutant(old, new, count=1):
    """EmuBackend with the forest entry points of a copy of this module in which `old` (found `count` times) reads `new`"""
    src = inspect.getsource(sys.modules[__name__]).split("\nfor _name, _fn in")[0]  # (without the attaching lines)
    assert src.count(old) == count, (old, src.count(old))
    ns = {"__name__": "emu_forest_mutant"}
    exec(compile(src.replace(old, new), "<emu_forest mutant>", "exec"), ns)
    return type("Mutant", (EmuBackend,), {k[1:]: v for k, v in ns.items() if k.startswith("_k_forest_")})()
