"""TEST INFRASTRUCTURE shared by tests/test_gpu_forest_diag.py (the HIP kernels, through the C-ABI) and
tests/test_forest_diag_emu.py (the numpy emulation, tests/emu_forest.py): case tables and a brute-force reference of
hypel_forest_oob_rows, hypel_forest_permuted_hits and hypel_forest_importances_f64.

Reference.  `ref_*` below: plain Python written from include/hypel.h alone -- the recursive walk and the vote of
tests/forest_kernel_cases.py, Python floats (IEEE double, one rounding per operation) for every vote and every importance
sum, each sum a literal loop in the order the header states.  It shares no code with tests/emu_forest.py and does
not import it.

Operands, `launch`, `run` and `settle` are those of tests/forest_kernel_cases.py: every pointer is an `Op` at an odd
offset inside sentinel bytes, every launch runs twice and must write the same bytes, and afterwards every byte of every
operand -- inputs and the unspecified parts of the outputs included -- equals what the reference left.  No tolerance
appears in this file."""
import numpy as np

from hypelcnn_amd import abi
from hypelcnn_amd.backend import FOREST_MAX_CLASSES, FOREST_NODE_DTYPE
from tests import forest_kernel_cases as K
from tests.forest_kernel_cases import F64, I32, U8, Op, launch, node_op, run, sent, settle

WINDOW = abi.const("HYPEL_FOREST_IMPORTANCE_WINDOW")
BLOCK = 256  # the chunk of nodes a workgroup of hypel_forest_importances_f64 takes at a time


# =============================================================================================== the reference (hypel.h)
def ref_oob_rows(x, ld, n, f, tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes, class_labels, weight,
                 ldw, out, proba, votes):
    rec = nodes.view(FOREST_NODE_DTYPE)[:n_nodes]
    for i in range(n):
        voting = [t for t in range(n_trees) if not int(weight[t * ldw + i]) > 0]
        mean, nv, win, _ = K.vote(rec, tree_off, leaf_value, n_classes, lambda c: x[i * ld + c], voting)
        proba[i * n_classes:(i + 1) * n_classes] = mean
        votes[i] = nv
        out[i] = win if class_labels is None else class_labels[win]


def ref_permuted_hits(x, ld, n, f, tree_off, n_trees, nodes, n_nodes, leaf_value, n_leaves, n_classes, y, partner,
                      n_repeats, group_mod, g0, n_groups, hits):
    rec = nodes.view(FOREST_NODE_DTYPE)[:n_nodes]
    for g in range(g0, g0 + n_groups):
        for r in range(n_repeats):
            for i in range(n):
                p = int(partner[r * n + i])
                read = lambda c: x[(p if c % group_mod == g else i) * ld + c]  # noqa: E731
                if K.vote(rec, tree_off, leaf_value, n_classes, read, range(n_trees))[2] == int(y[i]):
                    hits[(g - g0) * n_repeats + r] += 1


def ref_importances(nodes, n_nodes, tree_off, n_trees, value, n_classes, node_weight, impurity, f, per_tree,
                    importances, n_used):
    rec = nodes.view(FOREST_NODE_DTYPE)[:n_nodes]

    def imp(j):
        if impurity is not None:
            return float(impurity[j])
        s = 0.0
        for k in range(n_classes):
            v = float(value[j * n_classes + k])
            s = s + v * v
        return 1.0 - s

    def normalised(row):
        s = 0.0
        for v in row:
            s = s + v
        return [v / s for v in row] if s > 0 else row

    used, total = 0, [0.0] * f
    for t in range(n_trees):
        first, end = int(tree_off[t]), int(tree_off[t + 1]) if t + 1 < n_trees else n_nodes
        raw = [0.0] * f
        for j in range(first, end):
            c, l, r = int(rec["feature"][j]), int(rec["left"][j]), int(rec["right"][j])
            if l < 0:
                continue
            a, b, d = float(node_weight[j]) * imp(j), float(node_weight[l]) * imp(l), float(node_weight[r]) * imp(r)
            raw[c] = raw[c] + ((a - b) - d)
        row = normalised([v / float(node_weight[first]) for v in raw])
        per_tree[t * f:(t + 1) * f] = row
        if end - first > 1:
            used += 1
            total = [a + b for a, b in zip(total, row)]
    n_used[0] = used
    importances[:f] = normalised([v / float(used) for v in total]) if used else [0.0] * f


# ================================================================================================== 1. out-of-bag votes
#             n    C   trees (3: a chain, a balanced tree and a lone root)
OOB_CASES = [(1, 2, 1), (63, 2, 3), (64, 32, 3), (65, 2, 1), (257, 32, 3), (64, 2, 3), (257, 2, 1)]
F = 6


def model_and_rows(seed, n, n_classes, n_trees):
    rng = np.random.default_rng(seed)
    model = K.mixed_model(rng, F, n_classes, n_trees)
    x = K.serving_rows(rng, n, F)
    for i, level in enumerate(K.CHAIN_LEVELS[:n]):
        x[i, F - 1] = K.chain_value(level)
    return rng, model, x


def model_ops(model):
    rec, tree_off, leaves = model
    return (Op("tree_off", tree_off), len(tree_off), node_op("nodes", rec), len(rec), Op("leaf_value", leaves),
            len(leaves), leaves.shape[1])


def run_oob(be, n, n_classes, n_trees):
    """The chunk [3, 3 + n) of a table of n + 5 rows with ldw = n + 7: counts 0 .. 3, row 0 of the chunk in every bag,
    row 1 in no bag (its means must be those of hypel_forest_predict_rows); with and without class_labels"""
    rng, model, x = model_and_rows(7000 * n + 10 * n_classes + n_trees, n, n_classes, n_trees)
    ldw, r0 = n + 7, 3
    table = rng.integers(0, 4, (n_trees, ldw)).astype(I32)
    table[:, r0] = rng.integers(1, 4, n_trees)
    if n > 1:
        table[:, r0 + 1] = 0
    labels = (200 - 3 * np.arange(n_classes)).astype(U8)
    ld = F + 3
    for with_labels in (False, True):
        args = (Op("x", K.padded_rows(x, ld)), ld, n, F, *model_ops(model),
                Op("class_labels", labels) if with_labels else None, Op("weight", table.reshape(-1)[r0:]), ldw,
                Op("out", sent(U8, n + 3)), Op("proba", sent(F64, n * n_classes + 3)), Op("votes", sent(I32, n + 3)))
        run(be, "forest_oob_rows", ref_oob_rows, *args, tag=f"n{n} C{n_classes} trees{n_trees}")
    votes, proba = args[16].want, args[15].want
    assert votes[0] == 0 and not proba[:n_classes].any() and args[14].want[0] == labels[0]
    assert table.max() > 1
    if n > 1:
        pa = K.predict_args(x[1:2], ld, model, labels, None, 0, 0, True)
        ref = [a.want if isinstance(a, Op) else a for a in pa]
        K.ref_predict_rows(*ref)
        assert votes[1] == n_trees and np.array_equal(proba[n_classes:2 * n_classes], ref[15][:n_classes])
    if n >= 63:
        assert len(set(votes[2:n].tolist())) > 1


# ================================================================================================== 2. permuted hits
#              n    C  trees repeats group_mod g0 n_groups
HIT_CASES = [(1, 2, 1, 1, 1, 0, 1),
             (64, 2, 3, 3, 1, 0, 1),      # one group: every column comes from the partner row
             (63, 2, 3, 3, 6, 0, 6),      # every column its own group
             (64, 32, 3, 1, 4, 1, 3),     # 4 does not divide 6; a window of groups that starts at 1
             (65, 2, 1, 3, 6, 4, 2),      # one chain on the last column: group 4 is tested by no tree
             (257, 32, 3, 2, 8, 5, 3)]    # groups 6 and 7 hold no column: no tree tests them


def run_hits(be, n, n_classes, n_trees, n_repeats, group_mod, g0, n_groups):
    """y is the model's own winner for most rows; of three repeats the first is the identity partner; hits start from
    0 .. 3 (the launch adds).  Returns (hits the launch added, the baseline hits)"""
    rng, model, x = model_and_rows(9000 * n + n_repeats, n, n_classes, n_trees)
    rec, tree_off, leaves = model
    ld = F + 3
    win = [K.vote(rec, tree_off, leaves.reshape(-1), n_classes, lambda c: x[i, c], range(n_trees))[2] for i in range(n)]
    y = np.where(rng.random(n) < 0.7, win, rng.integers(0, n_classes, n)).astype(I32)
    identity = n_repeats >= 3
    partner = np.stack([np.arange(n)] * identity + [rng.permutation(n) for _ in range(n_repeats - identity)]).astype(I32)
    before = rng.integers(0, 4, n_groups * n_repeats + 3).astype(I32)
    args = (Op("x", K.padded_rows(x, ld)), ld, n, F, *model_ops(model), Op("y", y), Op("partner", partner), n_repeats,
            group_mod, g0, n_groups, Op("hits", before))
    run(be, "forest_permuted_hits", ref_permuted_hits, *args, tag=f"n{n} mod{group_mod} g0 {g0}")
    added = (args[17].want - before)[:n_groups * n_repeats].reshape(n_groups, n_repeats)
    baseline = int((np.array(win) == y).sum())
    if identity:
        assert (added[:, 0] == baseline).all()
    if n >= 63:
        assert (added != baseline).any()  # some permutation changed some winner
    assert (args[17].want[n_groups * n_repeats:] == before[n_groups * n_repeats:]).all()
    for g in range(g0, g0 + n_groups):
        tested = ((rec["left"] >= 0) & (rec["feature"] % group_mod == g)).any()
        if not tested:
            assert (added[g - g0] == baseline).all()
    return added, baseline


def run_hits_tree_order(be):
    """three stumps whose class sums depend on the order of the fp64 additions (the last of K.TIE_MODELS): every row is
    a hit in tree order, none in the reverse"""
    rows, winner = K.TIE_MODELS[-1]
    args = (Op("x", K.padded_rows(np.zeros((3, 1), np.float32), 2)), 2, 3, 1, *model_ops(K.stump_model(rows)),
            Op("y", np.full(3, winner, I32)), Op("partner", np.arange(3, dtype=I32)), 1, 1, 0, 1, Op("hits", np.zeros(1, I32)))
    run(be, "forest_permuted_hits", ref_permuted_hits, *args, tag="tree order")
    assert args[17].want[0] == 3


# ================================================================================================== 3. importances
IMPORTANCE_F = [1, 64, WINDOW, WINDOW + 1]


def comb(features):
    """a tree of len(features) inner nodes in a row, each with a leaf on its left: nodes 2k (inner, feature k-th),
    2k + 1 (its leaf), and a last leaf.  [] is a lone root."""
    n = len(features)
    rec = np.zeros(2 * n + 1, FOREST_NODE_DTYPE)
    rec["left"], rec["right"] = -1, 0
    for k, c in enumerate(features):
        rec[2 * k] = (c, 0.5, 2 * k + 1, 2 * k + 2)
    return rec


def importance_forest(f, seed=0):
    """0: BLOCK + 44 inner nodes all on the last column (the longest claim chain); 1: more nodes than one chunk, four
    columns interleaved, the window's edges among them; 2: a lone root; 3: every decrease 0 (pure nodes); 4: random
    columns.  Weights and class fractions are a tree's: a parent's are the sum and the weighted mean of its children's,
    so both impurities (Gini from value; the entropy, stored) are concave and no decrease is negative but by rounding."""
    rng = np.random.default_rng(f + seed)
    edge = (0, f // 2, min(f, WINDOW) - 1, f - 1)
    trees = [comb([f - 1] * (BLOCK + 44)), comb([edge[k % 4] for k in range(2 * BLOCK + 30)]), comb([]),
             comb(rng.integers(0, f, 10)), comb(rng.integers(0, f, 70))]
    weights, values = [], []
    for t, tree in enumerate(trees):
        w = rng.integers(1, 20, len(tree)).astype(F64) + rng.choice([0.0, 0.5], len(tree))
        v = rng.random((len(tree), 5)) + 0.01
        if t == 3:
            v[:] = [0.0, 1.0, 0.0, 0.0, 0.0]
        v /= v.sum(1, keepdims=True)
        for j in range(len(tree) - 1, -1, -1):
            l, r = int(tree["left"][j]), int(tree["right"][j])
            if l >= 0:
                w[j] = w[l] + w[r]
                v[j] = (w[l] * v[l] + w[r] * v[r]) / w[j]
        weights.append(w), values.append(v)
    off = np.cumsum([0] + [len(t) for t in trees])
    rec = np.concatenate(trees)
    inner = rec["left"] >= 0
    base = np.repeat(off[:-1], [len(t) for t in trees])
    rec["left"] = np.where(inner, rec["left"] + base, -1)
    rec["right"] = np.where(inner, rec["right"] + base, 0)
    value = np.concatenate(values)
    with np.errstate(divide="ignore", invalid="ignore"):
        impurity = -np.where(value > 0, value * np.log2(value), 0.0).sum(1)
    return rec, off[:-1].astype(I32), np.concatenate(weights), value, impurity


def importance_args(forest, f, given):
    rec, tree_off, weight, value, impurity = forest
    n_trees = len(tree_off)
    return (node_op("nodes", rec), len(rec), Op("tree_off", tree_off), n_trees, Op("value", value), value.shape[1],
            Op("node_weight", weight), Op("impurity", impurity) if given else None, f,
            Op("per_tree", sent(F64, (n_trees + 1) * f)), Op("importances", sent(F64, f + 3)), Op("n_used", sent(I32, 3)))


def run_importances(be, f, given):
    forest = importance_forest(f)
    args = importance_args(forest, f, given)
    run(be, "forest_importances_f64", ref_importances, *args, tag=f"f{f} impurity {'given' if given else 'NULL'}")
    per_tree, imp = args[9].want[:5 * f].reshape(5, f), args[10].want[:f]
    assert args[11].want[0] == 4 and not per_tree[2].any() and not per_tree[3].any()
    assert per_tree[0, f - 1] == 1.0 or f == 1
    assert abs(imp.sum() - 1.0) < 1e-12 and (per_tree[1] != 0).sum() == len({0, f // 2, min(f, WINDOW) - 1, f - 1})
    return args


def run_importances_lone_roots(be):
    """three lone roots: n_used 0, zeros everywhere"""
    rec = np.concatenate([comb([])] * 3)
    forest = (rec, np.arange(3, dtype=I32), np.array([5.0, 2.0, 9.0]), np.full((3, 2), 0.5), np.array([0.5, 0.5, 0.5]))
    for given in (True, False):
        args = importance_args(forest, 7, given)
        run(be, "forest_importances_f64", ref_importances, *args, tag="lone roots")
        assert args[11].want[0] == 0 and not args[10].want[:7].any() and not args[9].want[:21].any()


# ========================================================================================================== 4. refusals
def refusal_calls():
    """(label, kernel, args): valid small launches with one argument outside its contract; every output is sentinels"""
    rng, model, x = model_and_rows(5, 8, 2, 2)
    rec = model[0]
    calls = []

    def oob(label, **kw):
        a = [Op("x", K.padded_rows(x, 8)), 8, 8, F, *model_ops(model), None, Op("weight", np.zeros(2 * 8, I32)), 8,
             Op("out", sent(U8, 8)), Op("proba", sent(F64, 16)), Op("votes", sent(I32, 8))]
        for k, v in kw.items():
            a[dict(x=0, ld=1, nodes=6, C=10, weight=12, ldw=13, out=14, proba=15, votes=16)[k]] = v
        calls.append((label, "forest_oob_rows", tuple(a)))

    def hits(label, **kw):
        a = [Op("x", K.padded_rows(x, 8)), 8, 8, F, *model_ops(model), Op("y", np.zeros(8, I32)),
             Op("partner", np.arange(8, dtype=I32)), 1, F, 0, F, Op("hits", sent(I32, F))]
        for k, v in kw.items():
            a[dict(x=0, ld=1, nodes=6, C=10, y=11, partner=12, n_repeats=13, group_mod=14, g0=15, n_groups=16, hits=17)[k]] = v
        calls.append((label, "forest_permuted_hits", tuple(a)))

    forest = importance_forest(9)

    def imp(label, **kw):
        a = list(importance_args(forest, 9, False))
        for k, v in kw.items():
            a[dict(nodes=0, tree_off=2, value=4, C=5, node_weight=6, f=8, per_tree=9, importances=10, n_used=11)[k]] = v
        calls.append((label, "forest_importances_f64", tuple(a)))

    off = lambda r, lead: Op("nodes", r.view(U8), lead=lead)  # noqa: E731
    oob("x NULL", x=None), oob("weight NULL", weight=None), oob("out NULL", out=None), oob("proba NULL", proba=None)
    oob("votes NULL", votes=None), oob("n_classes 33", C=FOREST_MAX_CLASSES + 1), oob("ldw < n", ldw=7)
    oob("ld < f", ld=F - 1), oob("nodes 4 bytes off their alignment", nodes=off(rec, 52))
    hits("x NULL", x=None), hits("y NULL", y=None), hits("partner NULL", partner=None), hits("hits NULL", hits=None)
    hits("n_classes 33", C=FOREST_MAX_CLASSES + 1), hits("group_mod 0", group_mod=0), hits("group_mod -1", group_mod=-1)
    hits("n_repeats 0", n_repeats=0), hits("g0 + n_groups > group_mod", g0=1), hits("n_groups 0", n_groups=0)
    hits("nodes 8 bytes off their alignment", nodes=off(rec, 56))
    hits("a grid of 2^32 blocks", group_mod=1 << 30, n_groups=1 << 30, n_repeats=4)  # (refused: nothing is read)
    imp("nodes NULL", nodes=None), imp("tree_off NULL", tree_off=None), imp("node_weight NULL", node_weight=None)
    imp("value and impurity NULL", value=None), imp("n_classes 33 without impurity", C=FOREST_MAX_CLASSES + 1)
    imp("per_tree NULL", per_tree=None), imp("importances NULL", importances=None), imp("n_used NULL", n_used=None)
    imp("f 0", f=0), imp("nodes 4 bytes off their alignment", nodes=off(forest[0], 52))
    return calls


def run_refusals(be):
    for label, kernel, args in refusal_calls():
        launch(be, kernel, *args, refused=True)
        settle(kernel, *args, tag="refused: " + label)  # want = what was uploaded: not a byte has changed
