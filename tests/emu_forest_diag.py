"""TEST INFRASTRUCTURE: numpy twin of the forest diagnostics (include/hypel.h, hypel_forest_oob_rows,
hypel_forest_permuted_hits, hypel_forest_importances_f64), attached to tests/emu_backend.EmuBackend on import like
tests/emu_extra_trees.py.  Written from the header: the votes are fp64 additions in tree order (a tree that does not vote
adds nothing, not a zero), every importance sum is a sequential np.add.accumulate / np.add.at -- numpy's pairwise
np.sum is never used where the header fixes an order."""
import numpy as np

from hypelcnn_amd.backend import FOREST_MAX_CLASSES, FOREST_NODE_DTYPE
from tests.emu_backend import EmuBackend, _arr, _mat
from tests.emu_forest import _model, _write_labels
from tests.emu_scene import _typed


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


def vote(ends, leaf_value, voting):
    """(mean [n][C], votes [n], first maximum [n]) of the trees `voting` [n_trees][n] (bool), added in tree order"""
    total = np.zeros((ends.shape[1], leaf_value.shape[1]), np.float64)
    for t in range(ends.shape[0]):
        total[voting[t]] += leaf_value[ends[t][voting[t]]]
    votes = voting.sum(0).astype(np.int32)
    mean = np.zeros_like(total)
    np.divide(total, votes[:, None].astype(np.float64), out=mean, where=votes[:, None] > 0)
    return mean, votes, np.argmax(mean, 1)


def _k_forest_oob_rows(self, x, ld, n, f, tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes,
                       class_labels, weight, ldw, out, proba, votes):
    assert n > 0 and 0 < f <= ld and ldw >= n
    assert weight is not None and out is not None and proba is not None and votes is not None
    assert x is not None and tree_off is not None and nodes is not None and leaf_value is not None
    model = _model(tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes)
    m = _mat(x, ld, n, f)
    in_bag = _mat(weight, ldw, n_trees, n, np.int32)
    ends = leaf_rows(lambda rows, feat: m[rows, feat], *model[:6], n)
    mean, nv, win = vote(ends, model[6], ~(in_bag > 0))
    _typed(proba, np.float64, n * n_classes)[:] = mean.reshape(-1)
    _typed(votes, np.int32, n)[:] = nv
    _write_labels(win, class_labels, None, out, 0, n)


def _k_forest_permuted_hits(self, x, ld, n, f, tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes, y,
                            partner, n_repeats, group_mod, g0, n_groups, hits):
    assert n > 0 and 0 < f <= ld and n_repeats >= 1
    assert x is not None and y is not None and partner is not None and hits is not None
    assert tree_off is not None and nodes is not None and leaf_value is not None
    assert group_mod >= 1 and g0 >= 0 and n_groups >= 1 and g0 + n_groups <= group_mod
    assert n_groups * n_repeats * ((n + 63) // 64) < 1 << 31
    model = _model(tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes)
    m = _mat(x, ld, n, f)
    yv = _typed(y, np.int32, n)
    pt = _typed(partner, np.int32, n_repeats * n).reshape(n_repeats, n)
    h = _typed(hits, np.int32, n_groups * n_repeats).reshape(n_groups, n_repeats)
    everyone = np.ones((n_trees, n), bool)
    for g in range(g0, g0 + n_groups):
        cols = np.arange(f)[np.arange(f) % group_mod == g]
        for r in range(n_repeats):
            assert np.array_equal(np.sort(pt[r]), np.arange(n))
            mixed = m.copy()
            mixed[:, cols] = m[pt[r]][:, cols]
            ends = leaf_rows(lambda rows, feat: mixed[rows, feat], *model[:6], n)
            h[g - g0, r] += int((vote(ends, model[6], everyone)[2] == yv).sum())


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
