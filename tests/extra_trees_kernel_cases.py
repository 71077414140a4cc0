"""TEST INFRASTRUCTURE shared by tests/test_gpu_extra_trees_kernels.py (the HIP kernels, through the C-ABI) and
tests/test_extra_trees_kernel_cases_emu.py (the numpy emulation, tests/emu_forest.py): case tables and a brute-force
reference of hypel_forest_columns_f32, hypel_forest_split_random and hypel_forest_split_apply_thr.

Reference.  `ref_*` below: plain Python written from include/hypel.h alone -- np.float32 scalars for d, m and t (one
rounding per operation), Python ints for the class weights and the sums of squares, Python floats for the two divisions
and the addition.  It shares no code with tests/emu_forest.py and does not import it.  hypel_forest_split_apply_thr is
the one apply of tests/forest_kernel_cases.py: its reference, runners and tables serve both searches, here as K.CUTS.

Operands, `launch`, `run` and `settle` are those of tests/forest_kernel_cases.py: every pointer is an `Op` at an odd
offset inside sentinel bytes, every launch runs twice and must write the same bytes, and afterwards every byte of every
operand -- inputs and the unspecified parts of the outputs included -- equals what the reference left.  No tolerance
appears in this file.  No launch of the three caps its grid, so there is no case past a grid pass."""
import numpy as np

from hypelcnn_amd.backend import FOREST_MAX_CLASSES, FOREST_MAX_DEPTH
from tests import forest_kernel_cases as K
from tests.forest_kernel_cases import F32, F64, FLT_MAX, I32, Op, launch, run, sent, settle

U_TOP = np.nextafter(F32(1), F32(0))  # the largest float32 below 1
DENORMAL = F32(1e-45)


# =============================================================================================== the reference (hypel.h)
def ref_columns(x, ld, n, f, xt, ldn):
    for c in range(f):
        for i in range(n):
            xt[c * ldn + i] = F32(x[i * ld + c]) + F32(0.0)


def ref_cut(lo, hi, u):
    with np.errstate(over="ignore", invalid="ignore"):
        d = F32(hi - lo)
        m = F32(F32(u) * d)
        t = F32(lo + m)
    if not (t < hi):
        t = lo
    return t


def ref_split_random(xt, ldn, y, weight, n, n_classes, order, active, n_active, cand, u, max_features, f, score, thr,
                     valid, cuts=None):
    """cuts: a list that receives (record, lo, hi, t, rows going left, rows) of every valid record"""
    for a in range(n_active):
        tree, start, count = (int(v) for v in active[4 * a:4 * a + 3])
        rows = [int(order[start + i]) for i in range(count)]
        for s in range(max_features):
            at = a * max_features + s
            c = int(cand[at])
            score[at], thr[at], valid[at] = 0.0, 0.0, 0
            if count < 2:
                continue
            vals = [F32(xt[c * ldn + r]) for r in rows]
            lo, hi = min(vals), max(vals)
            if not (lo < hi):
                continue
            t = ref_cut(lo, hi, u[at])
            assert lo <= t < hi
            left, right = [0] * n_classes, [0] * n_classes
            for r, v in zip(rows, vals):
                (left if v <= t else right)[int(y[r])] += int(weight[tree * n + r])
            nl, nr = sum(left), sum(right)
            assert nl > 0 and nr > 0
            score[at] = float(sum(v * v for v in left)) / float(nl) + float(sum(v * v for v in right)) / float(nr)
            thr[at], valid[at] = t, 1
            if cuts is not None:
                cuts.append((at, lo, hi, t, sum(1 for v in vals if v <= t), count))


# ============================================================================================================ 1. columns
COLUMN_CASES = [(1, 1), (63, 5), (65, 33), (257, 3)]


def run_columns(be, n, f):
    """rows with ld > f into columns with ldn > n; column 0 holds both zeros; the row tails and the column past the
    last keep the sentinel"""
    rng = np.random.default_rng(10 * n + f)
    x = (rng.standard_normal((n, f)) * 100).astype(F32)
    x[:, 0] = rng.choice(np.array([-0.0, 0.0, 1.5], F32), n)
    x[0, 0] = -0.0
    if n > 1:
        x[1, 0] = 0.0
        x[-1, -1] = -FLT_MAX
    ld, ldn = f + 3, n + 5
    args = (Op("x", K.padded_rows(x, ld)), ld, n, f, Op("xt", sent(F32, (f + 1) * ldn)), ldn)
    run(be, "forest_columns_f32", ref_columns, *args, tag=f"n{n} f{f}")
    xt = args[4].want.reshape(f + 1, ldn)
    assert not np.signbit(xt[0, :n]).any() and np.signbit(x[:, 0]).any()
    assert np.array_equal(xt[:f, :n], x.T + F32(0))


# ======================================================================================================= 2. split_random
def random_ops(d, cand, u):
    mf = cand.shape[1]
    rec = d["n_active"] * mf + 3  # three records past the last stay untouched
    return (Op("xt", d["xt"]), d["ldn"], Op("y", d["y"]), Op("weight", d["weight"]), d["n"], d["C"],
            Op("order", d["order"]), Op("active", d["active"]), d["n_active"], Op("cand", cand), Op("u", u), mf, d["f"],
            Op("score", sent(F64, rec)), Op("thr", sent(F32, rec)), Op("valid", sent(I32, rec)))


ROW_COUNTS = [1, 2, 63, 64, 65, 256, 257, 1000]
#               name          counts                      C   mf  w_max
RANDOM_CASES = {
    "c2_mf1":     (ROW_COUNTS, 2, 1, 1),
    "c32_mff":    (ROW_COUNTS, 32, 5, 9),
    "c3_w9":      ([2, 3, 64, 65, 130], 3, 3, 9),
    "heavy_c2":   ([1000, 999, 513], 2, 5, 1 << 15),
    "600_nodes":  (None, 3, 3, 3),  # counts 2 .. 8, drawn
}


def random_scenario(name):
    counts, C, mf, w_max = RANDOM_CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    if counts is None:
        counts = [int(v) for v in rng.integers(2, 9, 600)]
    d = K.with_columns(K.scenario(rng, counts, C, w_max=w_max, zero=0), rng)
    if w_max > 9:
        d["weight"][...] = np.maximum(d["weight"], 1 << 14)
    if name == "c3_w9":  # few distinct values: many rows equal to the cut's neighbours, many equal lo
        d["xt"][:d["f"], :d["n"]] = rng.integers(-2, 3, (d["f"], d["n"])).astype(F32)
    cand = K.draw_cand(rng, len(counts), mf, d["f"])
    u = rng.random((len(counts), mf), dtype=F32)
    if name == "c3_w9":  # cuts that land exactly on a value of the column: `<=` is what is counted
        u = rng.choice(np.array([0.0, 0.25, 0.5, 0.75], F32), u.shape)
    return d, cand, u


def run_random(be, name):
    d, cand, u = random_scenario(name)
    args = random_ops(d, cand, u)
    cuts = []
    run(be, "forest_split_random", ref_split_random, *args, tag=name, cuts=cuts)
    assert len(cuts) >= (d["n_active"] - 1) * cand.shape[1] // 2
    if name == "heavy_c2":
        seg = d["segs"][0]
        assert d["weight"][0, seg].sum() > 1 << 24  # squares past int32
    return d, cand, args


# columns of the special case, one node after the other over disjoint rows
CONSTANT, ZEROS, FULL_RANGE, ONE_DENORMAL, ALL_BUT_ONE, ONE_ULP, PLAIN = range(7)
SPECIAL_COUNTS = [2, 16, 64, 65, 300, 2]


def special_scenario():
    rng = np.random.default_rng(77)
    d = K.disjoint_scenario(rng, SPECIAL_COUNTS, 2, 7, zero=0)
    K.with_columns(d, rng)
    for rows in d["segs"]:
        k = len(rows)
        first = rng.permutation(k)
        d["xt"][CONSTANT, rows] = 3.25
        d["xt"][ZEROS, rows] = np.where(first % 2 == 0, F32(-0.0), F32(0.0))
        d["xt"][FULL_RANGE, rows] = np.where(first == 0, -FLT_MAX, np.where(first == 1, FLT_MAX, rng.standard_normal(k)))
        d["xt"][ONE_DENORMAL, rows] = np.where(first % 2 == 0, F32(0.0), DENORMAL)
        d["xt"][ALL_BUT_ONE, rows] = np.where(first == 0, F32(10.0), rng.random(k).astype(F32))
        d["xt"][ONE_ULP, rows] = np.where(first % 2 == 0, F32(1.0), np.nextafter(F32(1.0), F32(2.0)))
    na = len(SPECIAL_COUNTS)
    cand = np.stack([rng.permutation(7) for _ in range(na)]).astype(I32)
    by_column = {ALL_BUT_ONE: F32(0.5), ONE_ULP: U_TOP}
    # even nodes: u = 0 (the cut is lo itself); odd nodes: the largest u; the two columns above keep theirs
    u = np.array([[by_column.get(int(c), F32(0.0) if a % 2 == 0 else U_TOP) for c in cand[a]] for a in range(na)], F32)
    return d, cand, u


def run_random_special(be):
    """a constant column and a column of both zeros (invalid); -FLT_MAX .. FLT_MAX (d = inf: u * d is inf, or NaN at
    u = 0 -- either way the cut falls back to lo); a column spanning one denormal; all rows but one going left; hi one
    ulp above lo with the largest u (lo + m rounds to hi: back to lo); u = 0 and u = the largest float32 below 1"""
    d, cand, u = special_scenario()
    args = random_ops(d, cand, u)
    cuts = []
    run(be, "forest_split_random", ref_split_random, *args, tag="special", cuts=cuts)
    thr, valid = args[14].want, args[15].want
    cuts = {c[0]: c for c in cuts}
    for a in range(len(SPECIAL_COUNTS)):
        for s, c in enumerate(cand[a]):
            at = a * 7 + s
            assert valid[at] == (c not in (CONSTANT, ZEROS)), (a, c)
            if not valid[at]:
                continue
            _, lo, hi, t, n_left, count = cuts[at]
            if c == FULL_RANGE:
                assert thr[at] == -FLT_MAX and n_left == 1
            if c == ONE_ULP:
                assert ref_cut(lo, hi, U_TOP) == lo and F32(lo + F32(U_TOP * F32(hi - lo))) == hi and thr[at] == F32(1.0)
            if c == ONE_DENORMAL:
                assert hi - lo == DENORMAL and thr[at] == 0.0
            if c == ALL_BUT_ONE:
                assert n_left == count - 1
            if c == PLAIN and a % 2 == 0:
                assert thr[at] == lo  # u = 0


# ================================================================================================== 3. split_apply_thr
def run_random_then_apply(be, name):
    """the tables hypel_forest_split_random wrote through hypel_forest_split_apply_thr: every training row lands on the
    side it was counted on"""
    d, cand, args = run_random(be, name)
    rec = d["n_active"] * cand.shape[1]
    o = K.run_apply(be, K.CUTS, d, cand, args[13].got[:rec], args[14].got[:rec], args[15].got[:rec], 0, 64,
                    d["n_active"] + 10, tag=name)
    assert o["splits"] > d["n_active"] // 2
    return o


# ========================================================================================================== 4. refusals
def refusal_calls():
    """(label, kernel, args): valid small launches with one argument outside its contract; every output is sentinels"""
    rng = np.random.default_rng(3)
    x = K.padded_rows((rng.standard_normal((8, 5))).astype(F32), 8)
    calls = []

    def columns(label, ld=8, ldn=8):
        calls.append((label, "forest_columns_f32", (Op("x", x), ld, 8, 5, Op("xt", sent(F32, 5 * 8)), ldn)))

    d = K.with_columns(K.scenario(rng, [8, 8], 2, zero=0), rng)
    cand = K.draw_cand(rng, 2, 2, d["f"])
    u = rng.random((2, 2), dtype=F32)

    def random(label, **kw):
        a = list(random_ops(d, cand, u))
        for k, v in kw.items():
            a[dict(ldn=1, C=5, mf=11)[k]] = v
        calls.append((label, "forest_split_random", tuple(a)))

    def apply(label, alias=False, **kw):
        o = K.node_ops(d, 12, 2)
        order_in = Op("order_in", d["order"])
        a = [Op("xt", d["xt"]), d["ldn"], Op("y", d["y"]), Op("weight", d["weight"]), d["n"], d["C"], order_in,
             order_in if alias else Op("order_out", sent(I32, d["order"].size)), Op("active", d["active"]), 2,
             Op("cand", cand), 2, d["f"], Op("score", np.ones(4)), Op("thr", np.zeros(4, F32)),
             Op("valid", np.ones(4, I32)), 0, 8, 8, 12, *o.values()]
        for k, v in kw.items():
            a[dict(ldn=1, C=5, mf=11, max_depth=17, cap=19)[k]] = v
        calls.append((label, "forest_split_apply_thr", tuple(a)))

    columns("ld < f", ld=4), columns("ldn < n", ldn=7)
    random("n_classes 0", C=0), random("n_classes 33", C=FOREST_MAX_CLASSES + 1)
    random("max_features > f", mf=d["f"] + 1), random("max_features 0", mf=0), random("ldn < n", ldn=d["n"] - 1)
    apply("n_classes 0", C=0), apply("n_classes 33", C=FOREST_MAX_CLASSES + 1), apply("max_features > f", mf=d["f"] + 1)
    apply("ldn < n", ldn=d["n"] - 1), apply("order_in == order_out", alias=True)
    apply("max_depth 65", max_depth=FOREST_MAX_DEPTH + 1), apply("node_capacity < node_base", cap=7)
    return calls


def run_refusals(be):
    for label, kernel, args in refusal_calls():
        launch(be, kernel, *args, refused=True)
        settle(kernel, *args, tag="refused: " + label)  # want = what was uploaded: not a byte has changed
