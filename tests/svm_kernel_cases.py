"""TEST INFRASTRUCTURE shared by tests/test_gpu_svm_kernels.py (the HIP kernels of csrc/svm.hip, through the C-ABI) and
tests/test_svm_kernel_cases_emu.py (the numpy twins, tests/emu_svm.py and tests/emu_svm_grid.py): case tables, operand
windows and the references of hypel_svm_smo_ovo, hypel_svm_smo_grid, hypel_svm_kernel_apply_f32,
hypel_svm_kernel_planes_f32, hypel_svm_vote and hypel_svm_vote_score.

The solver.  A device trajectory cannot in general be held bit for bit to numpy: csrc/svm.hip is compiled with fp
contraction, so `Ki[r] * di + Kj[r] * dj` may be one fma.  Two kinds of case get round that:
  rounding cases   arbitrary RBF / polynomial problems, judged by `certificate` alone: an optimality certificate written
                   from include/hypel.h and the dual problem, recomputed in np.longdouble from the K the solver read and
                   the five outputs it returned.  It shares no code with the twin (nothing below `certificate` and its
                   helpers touches tests.emu_svm) and does not care which trajectory led to the point it is shown.
  exact cases      K = I, K = 1 and a K of negative curvature: every intermediate is an integer or a small dyadic, an fma
                   and a multiply-add give the same bits, and the outputs are held byte for byte to closed forms and to the
                   twin.  Every selection of the identity cases is a full tie, so they pin "the last maximum wins" across
                   a thread's strided elements, lanes and waves.
Rounding cases run on both storage paths (LDS, and the caller's workspace at l_max = 2049) and must give the same bits.

Operands.  forest_kernel_cases.Op / launch: every pointer argument sits behind an odd sentinel lead and in front of a
sentinel tail, every launch runs twice from fresh uploads and must write the same bytes, and after it every operand, inputs
included, holds what the case says -- so the gaps of alpha_y, the slots past n_pairs, the pair table, K, and the parts of ws
outside [3 out_off, 3 (out_off + l)) of each pair still hold their sentinels.  `Op.windows` lists what a call may write."""
import functools
from collections import Counter

import numpy as np

import tests.emu_svm as E
import tests.emu_svm_grid  # noqa: F401 (attaches the grid-search twins to EmuBackend)
from hypelcnn_amd.backend import (SVM_CONVERGED, SVM_JOB_DTYPE, SVM_NOT_CONVERGED, SVM_PAIR_DTYPE, SVM_POLY, SVM_RBF)
from tests.forest_kernel_cases import Op, launch, same_bytes, sent, settle

F32, I32, U8, F64, LD = np.float32, np.int32, np.uint8, np.float64, np.longdouble
TOL, MAX_ITER, SEED = 1e-3, 20000, 7
EPS = 2.0 ** -50
LDS_L_MAX = 48 * 1024 // (3 * 8)  # 2048: the largest l_max whose alpha, gradient and diagonal fit the 48 KB of LDS
WS_L_MAX = LDS_L_MAX + 1
TAU = 1e-12  # include/hypel.h: libsvm's floor of a non-positive curvature


# ============================================================================================== the certificate (hypel.h)
def dual_sets(a, y, C):
    """libsvm's I_up and I_low of alpha >= 0"""
    return np.where(y > 0, a < C, a > 0), np.where(y > 0, a > 0, a < C)


def slack_of(K, C, max_iter):
    """how far a gradient updated incrementally in fp64 over at most max_iter steps can sit from the recomputed one,
    once for each of m and M: per step one rounding of a sum whose terms are bounded by l C max|K| (and of the 1)"""
    return 2.0 * EPS * max_iter * (1.0 + K.shape[0] * C * float(np.abs(K).max()))


def certificate(K, na, C, tol, max_iter, alpha_y, rho, obj, n_iter, status, optimum=None, tag=""):
    """K: the fp32 sub-matrix of the pair as the solver read it; alpha_y, rho, obj, n_iter, status: what it returned;
    optimum: (alpha_y*, f*) of the same problem at tol 1e-10.  Asserts
      the box       0 <= alpha <= C, and the sign of a nonzero alpha_y is the element's label
      the equality  |sum alpha_y| <= 2^-50 l C
      the stop      status CONVERGED: m(alpha) - M(alpha) <= tol + slack on G = y (K alpha_y) - 1 recomputed here, m the
                    maximum of -yG over I_up, M the minimum over I_low
      the objective |obj - (1/2 v'Kv - sum |v|)| <= 1e-9 |obj|, and
                    -1e-9 |f*| <= obj - f* <= (tol + slack) |alpha - alpha*|_1, the first-order bound of a convex dual at
                    a point whose KKT gap is at most tol + slack
      rho           libsvm's rule on the recomputed G (the mean of yG over the free elements, else (ub + lb) / 2),
                    within slack
      the cap       n_iter <= max_iter, and NOT_CONVERGED exactly when n_iter == max_iter
    Every bound is a property of fp64 and of the dual problem, none of the code under test.  Returns gap - tol."""
    l = K.shape[0]
    y = np.where(np.arange(l) < na, 1.0, -1.0)
    v = np.asarray(alpha_y, F64)
    a = v * y
    assert v.shape == (l,) and np.isfinite(v).all(), tag
    assert ((a >= 0) & (a <= C)).all(), f"{tag}: 0 <= alpha <= C and the sign of alpha_y is the label"
    assert abs(v.astype(LD).sum()) <= EPS * l * C, f"{tag}: sum alpha_y = {float(v.astype(LD).sum()):.3e}"
    assert 0 <= n_iter <= max_iter and status in (SVM_CONVERGED, SVM_NOT_CONVERGED), tag
    assert (status == SVM_NOT_CONVERGED) == (n_iter == max_iter), f"{tag}: status {status} after {n_iter} of {max_iter}"
    Kv = K.astype(LD) @ v.astype(LD)
    G = y * Kv - 1
    slack = slack_of(K, C, max_iter)
    up, low = dual_sets(a, y, C)
    m = (-y * G)[up].max() if up.any() else -np.inf
    M = (-y * G)[low].min() if low.any() else np.inf
    gap = float(m - M)
    if status == SVM_CONVERGED:
        assert gap <= tol + slack, f"{tag}: m - M = {gap:.6e} at a point reported converged (tol {tol:g})"
    f = float((v.astype(LD) * Kv).sum() / 2 - np.abs(v).astype(LD).sum())
    assert abs(obj - f) <= 1e-9 * abs(obj), f"{tag}: obj {obj!r}, recomputed {f!r}"
    if optimum is not None:
        v_opt, f_opt = optimum
        assert obj - f_opt >= -1e-9 * abs(f_opt), f"{tag}: obj {obj!r} below the optimum {f_opt!r}"
        if status == SVM_CONVERGED:
            room = (tol + slack) * float(np.abs(v - v_opt).sum())
            assert obj - f_opt <= room, f"{tag}: obj - f* = {obj - f_opt:.3e}, first-order bound {room:.3e}"
    yg = y * G
    free = (a > 0) & (a < C)
    if free.any():
        want = float(yg[free].sum() / free.sum())
    else:
        ub_set, lb_set = ((a >= C) & (y < 0)) | ((a <= 0) & (y > 0)), ((a >= C) & (y > 0)) | ((a <= 0) & (y < 0))
        ub = float(yg[ub_set].min()) if ub_set.any() else np.inf
        lb = float(yg[lb_set].max()) if lb_set.any() else -np.inf
        want = (ub + lb) / 2.0
    assert rho == want or abs(rho - want) <= slack, f"{tag}: rho {rho!r}, by libsvm's rule on the recomputed G {want!r}"
    return gap - tol


# ================================================================================================ the instrumented update
CLIPS = ("differ diff>0 aj<0", "differ diff<=0 ai<0", "differ diff>0 ai>C", "differ diff<=0 aj>C",
         "same sum>C ai>C", "same sum<=C aj<0", "same sum>C aj>C", "same sum<=C ai<0")


def count_events(K, na, C, tol, max_iter):
    """For counting only: libsvm's loop once more, with a Counter of what each step met -- "tau" (the curvature of the
    chosen pair was floored), "differ" / "same" (the label relation of (i, j)), the eight clip outcomes of CLIPS -- and
    the number of steps, which the emulation test holds equal to the twin's."""
    l = K.shape[0]
    K = K.astype(F64)
    y = np.where(np.arange(l) < na, 1.0, -1.0)
    alpha, G, seen, it = np.zeros(l), -np.ones(l), Counter(), 0
    last = lambda w: l - 1 - int(np.argmax(w[::-1]))  # noqa: E731
    while it < max_iter:
        up, low = dual_sets(alpha, y, C)
        if not up.any() or not low.any():
            break
        i = last(np.where(up, -y * G, -np.inf))
        gd = -y[i] * G[i] + y * G
        cand = low & (gd > 0)
        if -y[i] * G[i] + (y * G)[low].max() < tol or not cand.any():
            break
        raw = K[i, i] + np.diag(K) - 2.0 * K[i]
        quad = np.where(raw > 0, raw, TAU)
        j = last(np.where(cand, gd * gd / quad, -np.inf))
        seen["tau"] += int(not raw[j] > 0)
        ai0, aj0 = ai, aj = alpha[i], alpha[j]
        if y[i] != y[j]:
            seen["differ"] += 1
            delta, diff = (-G[i] - G[j]) / quad[j], ai - aj
            ai, aj = ai + delta, aj + delta
            if diff > 0 and aj < 0:
                seen[CLIPS[0]] += 1
                ai, aj = diff, 0.0
            elif diff <= 0 and ai < 0:
                seen[CLIPS[1]] += 1
                ai, aj = 0.0, -diff
            if diff > 0 and ai > C:
                seen[CLIPS[2]] += 1
                ai, aj = C, C - diff
            elif diff <= 0 and aj > C:
                seen[CLIPS[3]] += 1
                ai, aj = C + diff, C
        else:
            seen["same"] += 1
            delta, s = (G[i] - G[j]) / quad[j], ai + aj
            ai, aj = ai - delta, aj + delta
            if s > C and ai > C:
                seen[CLIPS[4]] += 1
                ai, aj = C, s - C
            elif s <= C and aj < 0:
                seen[CLIPS[5]] += 1
                ai, aj = s, 0.0
            if s > C and aj > C:
                seen[CLIPS[6]] += 1
                ai, aj = s - C, C
            elif s <= C and ai < 0:
                seen[CLIPS[7]] += 1
                ai, aj = 0.0, s
        alpha[i], alpha[j] = ai, aj
        G += y * (K[i] * ((ai - ai0) * y[i]) + K[j] * ((aj - aj0) * y[j]))
        it += 1
    return seen, it


# ========================================================================================================== the problems
class Problem:
    """One pair problem: K [l][l] fp32 in element order (the na elements of y = +1 first), and what it is solved with."""

    def __init__(self, name, K, na, C, max_iter=MAX_ITER, closed=None):
        self.name, self.K, self.na, self.nb, self.l, self.C = name, np.ascontiguousarray(K, F32), na, len(K) - na, len(K), C
        self.max_iter, self.closed = max_iter, closed

    @functools.cached_property
    def twin(self):
        """(alpha_y, rho, obj, n_iter, status) of tests.emu_svm.smo_pair"""
        return E.smo_pair(self.K, self.na, self.C, TOL, self.max_iter)

    @functools.cached_property
    def optimum(self):
        """(alpha_y*, f*): the twin at tol 1e-10, for the certificate's objective bound"""
        ay, _, f, _, status = E.smo_pair(self.K, self.na, self.C, 1e-10, E.SVM_MAX_ITER_LIMIT)
        assert status == SVM_CONVERGED, self.name
        return ay, f

    @functools.cached_property
    def twin_margin(self):
        """gap - tol of the twin's own result, by the certificate"""
        return certificate(self.K, self.na, self.C, TOL, self.max_iter, *self.twin, optimum=self.optimum,
                           tag=self.name + " (twin)")

    @functools.cached_property
    def events(self):
        return count_events(self.K, self.na, self.C, TOL, self.max_iter)


def two_classes(seed, na, nb, dim=6, shift=0.7):
    rng = np.random.default_rng([SEED, seed])
    return rng.standard_normal((na + nb, dim)) + (np.arange(na + nb) >= na)[:, None] * shift


def rbf(x, gamma=0.3):
    return np.exp(-gamma * ((x[:, None] - x[None]) ** 2).sum(2)).astype(F32)


def with_copies(x, na, n_copies):
    """the first n_copies rows of the second class are exact copies of rows of the first: quad is exactly 0 there"""
    x = x.copy()
    x[na:na + n_copies] = x[:n_copies]
    return x


def labels(na, nb):
    return np.where(np.arange(na + nb) < na, 1.0, -1.0)


def identity_closed(na, nb, k):
    """K = I after k <= min(na, nb) steps: every selection is a full tie, both resolve to the largest index"""
    a = np.zeros(na + nb)
    a[na - k:na] = a[na + nb - k:] = 1.0
    return a * labels(na, nb), 0.0, -float(k), k, SVM_NOT_CONVERGED


def constant_closed(na, nb, C):
    """K = 1, na < nb: every curvature is 0, every step takes the TAU floor and clips both multipliers to C"""
    a = np.zeros(na + nb)
    a[:na] = a[nb:] = C
    return a * labels(na, nb), 1.0, -2.0 * na * C, na, SVM_CONVERGED


def negative_curvature(na, nb):
    """1 inside a class and on the diagonal, 2 across the classes: quad = 1 + 1 - 4 < 0 for every pair of unlike labels.
    Integers throughout (no closed form is claimed: the twin is the reference).  Without the floor the first step has
    delta = 2 / -2, both multipliers clip back to 0 and the solver spins to the cap."""
    K = np.ones((na + nb, na + nb), F32)
    K[:na, na:] = K[na:, :na] = 2.0
    return K


@functools.lru_cache(maxsize=None)
def problems():
    x95 = two_classes(0, 40, 55)
    eye = lambda n: np.eye(n, dtype=F32)  # noqa: E731
    p = [Problem(f"rbf95_C{C:g}", rbf(x95), 40, C) for C in (1e-2, 1.0, 1e3)]
    p += [Problem("all_at_C", rbf(two_classes(1, 64, 64)), 64, 1e-2),
          Problem("one_row_class", rbf(two_classes(2, 1, 300)), 1, 10.0),
          Problem("l257", rbf(two_classes(3, 129, 128)), 129, 10.0),
          Problem("l513", rbf(two_classes(4, 300, 213)), 300, 100.0),
          Problem("copies", rbf(with_copies(two_classes(5, 50, 50), 50, 20)), 50, 5.0)]
    x = two_classes(6, 45, 45)
    p += [Problem("poly3", ((0.2 * (x @ x.T) + 1.0) ** 3).astype(F32), 45, 1.0)]
    p += [Problem(f"identity_k{k}", eye(300), 130, 4.0, k, identity_closed(130, 170, k)) for k in (1, 7, 130)]
    p += [Problem("constant", np.ones((127, 127), F32), 37, 2.0, 50, constant_closed(37, 90, 2.0)),
          Problem("negative_curvature", negative_curvature(5, 9), 5, 2.0, 50),
          Problem("identity_2048", eye(2048), 1024, 4.0, 64, identity_closed(1024, 1024, 64)),
          Problem("identity_2049", eye(2049), 1025, 4.0, 64, identity_closed(1025, 1024, 64)),
          Problem("identity_free", eye(300), 130, 4.0)]  # (to convergence: dyadic fractions, exact against the twin)
    return {q.name: q for q in p}


#                 group        problems                              exact
SOLVER_GROUPS = {
    "C1e-2":      (("rbf95_C0.01", "all_at_C"), False),
    "C1":         (("rbf95_C1", "poly3"), False),
    "C1e3":       (("rbf95_C1000",), False),
    "C10":        (("one_row_class", "l257"), False),
    "C100":       (("l513",), False),
    "C5":         (("copies",), False),
    "identity1":  (("identity_k1",), True),
    "identity7":  (("identity_k7",), True),
    "identity130": (("identity_k130",), True),
    "tau":        (("constant", "negative_curvature"), True),
    "lds_limit":  (("identity_2048",), True),
    "past_lds":   (("identity_2049",), True),
}
ROUNDING_GROUPS = [g for g, (_, exact) in SOLVER_GROUPS.items() if not exact]
EXACT_GROUPS = [g for g, (_, exact) in SOLVER_GROUPS.items() if exact]


# ====================================================================================================== solver launches
class Layout:
    """The problems of one launch inside one K [rows][ldk] (NaN wherever no pair reads), each with its two classes in
    ranges of their own -- every other problem with the y = -1 rows in front of the y = +1 rows -- a pair table that is not
    in the order of the rows, and out_off in yet another order with gaps between the pairs."""

    def __init__(self, probs, lead_rows=3):
        self.probs = probs
        n = len(probs)
        at, spans = lead_rows, []
        for k, q in enumerate(probs):
            a0, b0 = (at + q.nb + 1, at) if k % 2 else (at, at + q.na + 2)
            spans.append((a0, b0))
            at += q.l + 5
        self.rows, self.ldk = at, at + 3
        self.K = np.full((self.rows, self.ldk), np.nan, F32)
        self.table = np.zeros(n, SVM_PAIR_DTYPE)
        self.slot = list(range(n))[::-1] if n > 1 else [0]  # pair p of the table is problem slot[p]
        offs, off = {}, 2
        for k in list(range(1, n)) + [0]:  # the first problem's outputs lie last
            offs[k] = off
            off += probs[k].l + 1 + k % 2 * 2
        self.total = off + 3
        for p, k in enumerate(self.slot):
            q, (a0, b0) = probs[k], spans[k]
            idx = self.elements(a0, q.na, b0, q.nb)
            self.K[np.ix_(idx, idx)] = q.K
            self.table[p] = (a0, q.na, b0, q.nb, offs[k])

    @staticmethod
    def elements(a0, na, b0, nb):
        return np.concatenate([np.arange(a0, a0 + na), np.arange(b0, b0 + nb)])

    def sub(self, p):
        """the pair's K as the solver reads it"""
        r = self.table[p]
        idx = self.elements(int(r["a0"]), int(r["na"]), int(r["b0"]), int(r["nb"]))
        return self.K[np.ix_(idx, idx)]


def out_ops(n, total, with_ws):
    """alpha_y, rho, obj, n_iter, status, ws of n problems: sentinels, three slots past the last problem"""
    return [Op("alpha_y", sent(F64, total)), Op("rho", sent(F64, n + 3)), Op("obj", sent(F64, n + 3)),
            Op("n_iter", sent(I32, n + 3)), Op("status", sent(I32, n + 3)),
            Op("ws", sent(F64, 3 * total)) if with_ws else None]


def take(outs, table):
    """What a launch may have written, copied from `got` into `want` (whatever lies outside keeps its sentinel and is
    compared by settle), and the outputs per record of the pair or job table: [(alpha_y, rho, obj, n_iter, status)]"""
    ay, rho, obj, it, st, ws = outs
    res = []
    for o in outs:
        if o is not None:
            o.windows = []
    for at, r in enumerate(table):
        off, l = int(r["out_off"]), int(r["na"]) + int(r["nb"])
        for o, lo, hi in ((ay, off, off + l), (rho, at, at + 1), (obj, at, at + 1), (it, at, at + 1), (st, at, at + 1)) + \
                (((ws, 3 * off, 3 * (off + l)),) if ws is not None else ()):
            o.want[lo:hi] = o.got[lo:hi]
            o.windows.append((lo, hi))
        res.append((ay.got[off:off + l].copy(), float(rho.got[at]), float(obj.got[at]), int(it.got[at]), int(st.got[at])))
    return res


def launch_ovo(be, lay, C, max_iter, l_max, with_ws, refused=False):
    outs = out_ops(len(lay.table), lay.total, with_ws)
    args = (Op("k", lay.K), lay.ldk, Op("pairs", lay.table.view(U8), lead=SVM_PAIR_DTYPE.itemsize), len(lay.table), l_max,
            C, TOL, max_iter, *outs)
    launch(be, "svm_smo_ovo", *args, refused=refused)
    res = None if refused else take(outs, lay.table)
    settle("svm_smo_ovo", *args, tag=f"l_max {l_max}")
    return res


def same_result(tag, got, want):
    for name, g, w in zip(("alpha_y", "rho", "obj", "n_iter", "status"), got, want):
        same_bytes(f"{tag} {name}", np.asarray(g), np.asarray(w, np.asarray(g).dtype))


def run_solver_group(be, group):
    """One launch of the group's problems; the rounding groups once more on the workspace path (l_max = 2049 only sizes
    storage: the same bits).  Prints gap - tol and the iterations of every rounding problem beside the twin's."""
    names, exact = SOLVER_GROUPS[group]
    probs = [problems()[n] for n in names]
    lay = Layout(probs)
    C, max_iter = probs[0].C, probs[0].max_iter
    assert all(q.C == C and q.max_iter == max_iter for q in probs)
    l_max = max(q.l for q in probs)
    if l_max > LDS_L_MAX:
        launch_ovo(be, lay, C, max_iter, l_max, False, refused=True)  # beyond the LDS budget without a workspace
    res = launch_ovo(be, lay, C, max_iter, l_max, l_max > LDS_L_MAX)
    if not exact:
        for p, (r, w) in enumerate(zip(res, launch_ovo(be, lay, C, max_iter, WS_L_MAX, True))):
            same_result(f"{probs[lay.slot[p]].name}: workspace against LDS,", w, r)
    for p, r in enumerate(res):
        q = probs[lay.slot[p]]
        if exact:
            same_result(f"{q.name}: against the twin,", r, q.twin)
            if q.closed is not None:
                same_result(f"{q.name}: against the closed form,", r, q.closed)
        else:
            margin = certificate(lay.sub(p), q.na, C, TOL, max_iter, *r, optimum=q.optimum, tag=q.name)
            print(f"{q.name}: gap - tol {margin:+.3e} after {r[3]} iterations (twin {q.twin_margin:+.3e} after {q.twin[3]})")
    return res


GRID_JOBS = ("identity_free", "constant", "rbf95_C1", "l257")
GRID_JOBS_SHORT = ("negative_curvature", "constant", "rbf95_C0.01", "all_at_C")  # (for the stray-write checks)
EXACT_NAMES = {n for g in EXACT_GROUPS for n in SOLVER_GROUPS[g][0]} | {"identity_free"}


def run_grid(be, names=GRID_JOBS):
    """hypel_svm_smo_grid: exact and rounding problems as the jobs of one launch -- two planes of K, every job its own c
    and k_off, a permuted order -- on both storage paths, bit-equal to each job's own hypel_svm_smo_ovo launch"""
    probs = [problems()[n] for n in names]
    lays = [Layout(probs[:2]), Layout(probs[2:], lead_rows=1)]
    ldk = max(lay.ldk for lay in lays)
    planes, k_off = [], []
    for lay in lays:
        plane = np.full((lay.rows + 1, ldk), np.nan, F32)
        plane[:lay.rows, :lay.ldk] = lay.K
        k_off.append(5 + sum(p.size for p in planes))
        planes.append(plane)
    K = np.concatenate([np.full(5, np.nan, F32)] + [p.reshape(-1) for p in planes])
    jobs, owner, total = np.zeros(len(probs), SVM_JOB_DTYPE), [], 1
    order = np.array([2, 0, 3, 1], I32)
    for j, (which, p) in enumerate(((1, 0), (0, 1), (0, 0), (1, 1))):  # (plane, pair of its table)
        r, q = lays[which].table[p], lays[which].probs[lays[which].slot[p]]
        jobs[j] = (r["a0"], r["na"], r["b0"], r["nb"], total, k_off[which], q.C)
        total += q.l + 2
        owner.append(q)
    assert len({q.C for q in owner}) == len(owner) or names is not GRID_JOBS
    assert len(set(k_off)) == 2
    runs = []
    for l_max in (max(q.l for q in owner), WS_L_MAX):
        outs = out_ops(len(jobs), total, l_max > LDS_L_MAX)
        args = (Op("k", K), ldk, Op("jobs", jobs.view(U8), lead=SVM_JOB_DTYPE.itemsize), Op("order", order), len(jobs),
                l_max, TOL, MAX_ITER, *outs)
        launch(be, "svm_smo_grid", *args)
        runs.append(take(outs, jobs))
        settle("svm_smo_grid", *args, tag=f"l_max {l_max}")
    for j, q in enumerate(owner):
        same_result(f"smo_grid job {j} ({q.name}): workspace against LDS,", runs[1][j], runs[0][j])
        one = np.zeros(1, SVM_PAIR_DTYPE)
        one[0] = tuple(jobs[j][f] for f in ("a0", "na", "b0", "nb")) + (2,)
        outs = out_ops(1, q.l + 4, False)
        args = (Op("k", K[int(jobs[j]["k_off"]):], lead=int(jobs[j]["k_off"]) % 4 + 1), ldk,
                Op("pairs", one.view(U8), lead=SVM_PAIR_DTYPE.itemsize), 1, q.l, q.C, TOL, MAX_ITER, *outs)
        launch(be, "svm_smo_ovo", *args)
        same_result(f"smo_grid job {j} ({q.name}): against its smo_ovo launch,", runs[0][j], take(outs, one)[0])
        settle("svm_smo_ovo", *args)
        if q.name in EXACT_NAMES:
            same_result(f"smo_grid job {j} ({q.name}): against the twin,", runs[0][j], q.twin)
    return runs[0]


# ========================================================================================================= kernel values
def padded(x, ld):
    out = sent(x.dtype, x.shape[0] * ld).reshape(x.shape[0], ld)
    out[:, :x.shape[1]] = x
    return out


@functools.lru_cache(maxsize=None)
def value_inputs():
    """name -> (g [rows][cols], kind, gamma, coef0, degree, row_norms, col_norms)"""
    rng = np.random.default_rng([SEED, 100])
    x = (rng.standard_normal((37, 9)) * 3e3).astype(F32).astype(F64)
    norms = (x * x).sum(1)
    # the self-products as a GEMM stores them: fp32 roundings of |x|^2, so norms + norms - 2 g lies a few units either side
    # of 0
    cases = {"diagonal": ((x @ x.T).astype(F32), SVM_RBF, 0.05, 0.0, 0, norms, norms)}
    # gamma d2 = 80 (a normal result), 88 and 95 (fp32 denormals), 103.9 (just above half the smallest denormal) and 110
    # (zero) in column 0; the other columns a little beside them
    places = np.array([80.0, 88.0, 95.0, 103.9, 110.0, 87.3365, 103.28])  # (87.3365: the smallest normal; 103.28: 2^-149)
    g = np.zeros((len(places), 5), F32)
    g[:, 1:] = rng.standard_normal((len(places), 4)) * 0.01
    cases["tail"] = (g, SVM_RBF, 0.5, 0.0, 0, places / 0.5, np.arange(5) * 2.0 ** -6)
    g = (rng.standard_normal((23, 5)) * 3).astype(F32)
    cases["poly2"] = (g, SVM_POLY, 0.25, 1.0, 2, None, None)  # gamma g + coef0 is exact: an fma changes nothing
    cases["poly1"] = (np.abs(g), SVM_POLY, 0.37, 0.6, 1, None, None)  # (no cancellation: the one rounding an fma saves
    cases["poly3"] = (np.abs(g), SVM_POLY, 0.37, 0.6, 3, None, None)  # is 2^-53 of the value)
    g = np.array([[1e13, -1e13, 3e12, 6.9e12, 1.0], [-3e12, 7e12, -7e12, 0.0, -1e13]], F32)
    cases["poly3_overflow"] = (g, SVM_POLY, 1.0, 0.0, 3, None, None)  # beyond FLT_MAX = 3.4e38: +-inf
    return cases


def want_values(g, kind, gamma, coef0, degree, rn, cn):
    with np.errstate(over="ignore"):
        return E.kernel_values(g, kind, gamma, coef0, degree, rn, cn)


def check_values(tag, got, want64):
    """|got - want64| <= (0.5 + 2^-20) ulp of the fp32 result: half an ulp of the one rounding to fp32, and the fp64
    library's exp (1 ulp of fp64 is 2^-29 of an fp32 ulp) -- in units of the spacing, so that denormals count"""
    with np.errstate(over="ignore", invalid="ignore"):
        want32 = want64.astype(F32)
        big = np.isinf(want32)
        assert np.array_equal(got[big], want32[big]), f"{tag}: beyond FLT_MAX"
        err = np.abs(got.astype(F64) - want64)[~big]
        room = (0.5 + 2.0 ** -20) * np.spacing(np.abs(want32[~big])).astype(F64)
    worst = float((err / room).max())
    assert (err <= room).all(), f"{tag}: {int((err > room).sum())} values off by up to {worst:.3f} of the bound"


#              name       lead  ld(cols)
VALUE_FORMS = {"vector":     (8, lambda cols: (cols + 4) // 4 * 4),       # a pad column at least, whole quads
               "misaligned": (7, lambda cols: (cols + 4) // 4 * 4),       # one float off 16 bytes: the scalar form
               "odd_ld":     (8, lambda cols: (cols + 1) | 1)}
VALUE_COLS = (1, 3, 4, 5)


def apply_launch(be, g, ld, lead, spec, rows=None, refused=False):
    kind, gamma, coef0, degree, rn, cn = spec
    rows = g.shape[0] if rows is None else rows
    op = Op("g", padded(g, ld), lead=lead)
    args = (op, ld, rows, g.shape[1], kind, gamma, coef0, degree, None if rn is None else Op("row_norms", rn),
            None if cn is None else Op("col_norms", cn))
    launch(be, "svm_kernel_apply_f32", *args, refused=refused)
    got = op.got.reshape(g.shape[0], ld)[:rows, :g.shape[1]].copy()
    op.want.reshape(g.shape[0], ld)[:rows, :g.shape[1]] = got
    op.windows = [(r * ld, r * ld + g.shape[1]) for r in range(rows)]
    settle("svm_kernel_apply_f32", *args)
    return got


def run_values(be, name):
    """hypel_svm_kernel_apply_f32 in its three forms on 1, 3, 4 and 5 columns (the diagonal case: on all 37) against the
    float64 kernel_values, the forms against each other bit for bit; rows = 0 writes nothing"""
    g, *spec = value_inputs()[name]
    kind, gamma, coef0, degree, rn, cn = spec
    seen = []
    for cols in (g.shape[1],) if name == "diagonal" else VALUE_COLS:
        part = np.ascontiguousarray(g[:, :cols])
        sp = (kind, gamma, coef0, degree, rn, None if cn is None else cn[:cols])
        want64 = want_values(part, *sp)
        first = None
        for form, (lead, ld_of) in VALUE_FORMS.items():
            ld = ld_of(cols)
            assert (form == "vector") == (ld % 4 == 0 and lead % 4 == 0) and ld > cols
            got = apply_launch(be, part, ld, lead, sp)
            check_values(f"kernel_apply {name} cols {cols} {form}", got, want64)
            first = got if first is None else first
            same_bytes(f"kernel_apply {name} cols {cols}: {form} against the vector form", got, first)
        seen.append((first, want64))
        apply_launch(be, part, ld_of(cols), 8, sp, rows=0)
    if name == "diagonal":
        d2 = rn[:, None] + cn[None, :] - 2.0 * g.astype(F64)
        below = np.diag(d2) <= 0
        assert 5 <= below.sum() <= len(below) - 5 and (np.diag(d2)[~below] * gamma > 1e-3).all()
        assert (np.diag(seen[0][0])[below] == F32(1.0)).all() and (np.diag(seen[0][0])[~below] < F32(1.0)).all()
    if name == "tail":
        got = seen[-1][0][:, 0]
        tiny = float(np.finfo(F32).tiny)
        assert got[0] >= tiny and (0 < got[1:4]).all() and (got[1:4] < tiny).all() and got[4] == 0, got  # denormals are kept
        assert got[3] == got[6] == F32(2.0 ** -149)
    if name == "poly3_overflow":
        assert np.isinf(seen[-1][0]).sum() == 5 and np.isfinite(seen[-1][0]).sum() == 5
    return seen


def planes_launch(be, g, ld, lead, gammas, rn, cn, stride_pad, rows=None, refused=False, out=None, stride=None):
    rows = g.shape[0] if rows is None else rows
    stride = g.shape[0] * ld + stride_pad if stride is None else stride
    gop = Op("g", padded(g, ld), lead=lead)
    oop = gop if out == "g" else Op("out", sent(F32, (len(gammas) - 1) * stride + g.shape[0] * ld + 3), lead=lead)
    args = (gop, ld, rows, g.shape[1], SVM_RBF, Op("gammas", np.asarray(gammas, F64)), len(gammas), Op("row_norms", rn),
            Op("col_norms", cn), oop, stride)
    launch(be, "svm_kernel_planes_f32", *args, refused=refused)
    planes, oop.windows = [], []
    for p in range(len(gammas) if not refused else 0):
        view = lambda a: a[p * stride:p * stride + g.shape[0] * ld].reshape(g.shape[0], ld)[:rows, :g.shape[1]]  # noqa: E731
        planes.append(view(oop.got).copy())
        view(oop.want)[...] = planes[-1]
        oop.windows += [(p * stride + r * ld, p * stride + r * ld + g.shape[1]) for r in range(rows)]
    settle("svm_kernel_planes_f32", *args)
    return planes


def run_planes(be, name):
    """hypel_svm_kernel_planes_f32 on the RBF inputs, vector and scalar forms: every plane the bits of kernel_apply with
    that gamma, g, the pad columns and what lies between and behind the planes untouched"""
    g, kind, gamma, _, _, rn, cn = value_inputs()[name]
    gammas = [gamma, 2.0 * gamma, gamma / 3.0]
    cols = g.shape[1]
    want = [apply_launch(be, g, cols + 3, 8, (SVM_RBF, gam, 0.0, 0, rn, cn)) for gam in gammas]
    for form, lead, ld, pad in (("vector", 8, (cols + 4) // 4 * 4, 4), ("misaligned", 7, (cols + 4) // 4 * 4, 4),
                                ("odd_stride", 8, (cols + 4) // 4 * 4, 5)):
        planes = planes_launch(be, g, ld, lead, gammas, rn, cn, pad)
        for p, plane in enumerate(planes):
            same_bytes(f"kernel_planes {name} {form} plane {p} against kernel_apply", plane, want[p])
    planes_launch(be, g, cols + 3, 8, gammas, rn, cn, 2, rows=0)


def value_refusals(be):
    g, _, gamma, _, _, rn, cn = value_inputs()["tail"]
    poly = (SVM_POLY, 0.5, 1.0)
    labels = []
    for label, spec in (("degree 0", (*poly, 0, None, None)), ("degree 4", (*poly, 4, None, None)),
                        ("rbf without row norms", (SVM_RBF, gamma, 0.0, 0, None, cn)),
                        ("rbf without col norms", (SVM_RBF, gamma, 0.0, 0, rn, None)),
                        ("rbf without norms", (SVM_RBF, gamma, 0.0, 0, None, None)),
                        ("kind 2", (2, gamma, 0.0, 1, rn, cn))):
        apply_launch(be, g, 8, 8, spec, refused=True)
        labels.append(label)
    planes_launch(be, g, 8, 8, [gamma, 1.0], rn, cn, 0, refused=True, stride=g.shape[0] * 8 - 1)
    planes_launch(be, g, 8, 8, [gamma], rn, cn, 0, refused=True, out="g")
    return labels + ["overlapping planes", "in place"]


# ================================================================================================================== votes
VOTE_CLASSES, VOTE_ROWS = 256, 300
DEC_VALUES = np.array([-1, 0, 0.0, 1, -0.0, 1e-30, -1e-30, np.nan, np.inf, -np.inf], F32)


def sweep_rows(dec, n_classes, winners):
    """row k of dec: class winners[k] wins every one of its n_classes - 1 pairs"""
    a, b = np.triu_indices(n_classes, 1)
    for k, w in enumerate(winners):
        dec[k, :len(a)][a == w] = 1e-30
        dec[k, :len(a)][b == w] = -0.0


@functools.lru_cache(maxsize=None)
def vote_decisions(n_classes=VOTE_CLASSES, rows=VOTE_ROWS, pad=5):
    """dec [rows][n_pairs + pad]: rows 0 .. 3 a class with all n_classes - 1 votes (a byte counter at 255 when there are
    256 classes), then rows of NaN, of -0.0 (every vote to the higher class: the last class takes them all) and of +1 (the
    first class does); the rest drawn from DEC_VALUES, the pad columns included.  -> (dec, the winners by E.vote)"""
    rng = np.random.default_rng([SEED, n_classes])
    n_pairs = n_classes * (n_classes - 1) // 2
    dec = rng.choice(DEC_VALUES, (rows, n_pairs + pad))
    sweep_rows(dec, n_classes, (0, n_classes - 1, 100, 1))
    dec[4, :n_pairs], dec[5, :n_pairs], dec[6, :n_pairs] = np.nan, -0.0, 1.0
    win = E.vote(dec[:, :n_pairs], n_classes)
    assert list(win[:7]) == [0, n_classes - 1, 100, 1, n_classes - 1, n_classes - 1, 0]
    return dec, win


def run_vote(be, with_labels, with_points):
    n, rows = VOTE_CLASSES, VOTE_ROWS
    dec, win = vote_decisions()
    labels = ((np.arange(n) * 37 + 11) % 256).astype(U8)
    w, h = 23, rows // 23 + 2
    at = np.random.default_rng(rows).permutation(w * h)[:rows]
    points = np.stack([at % w, at // w], 1).astype(I32)
    raster_w = w + 2
    out = Op("out", sent(U8, raster_w * h if with_points else rows + 3))
    lab = labels[win] if with_labels else win.astype(U8)
    where = points[:, 1] * raster_w + points[:, 0] if with_points else np.arange(rows)
    out.want[where] = lab
    out.windows = [(int(k), int(k) + 1) for k in where]
    args = (Op("dec", dec), dec.shape[1], rows, n, Op("class_labels", labels) if with_labels else None,
            Op("points", points) if with_points else None, out, raster_w if with_points else 0)
    launch(be, "svm_vote", *args)
    settle("svm_vote", *args, tag=f"labels {with_labels} points {with_points}")


SCORE_CLASSES, SCORE_CELLS, SCORE_ROWS = 255, 3, 40


def run_vote_score(be):
    """hypel_svm_vote_score at its 255 classes: correct[cell] += the rows whose winner by E.vote is truth[r], and the same
    counts from hypel_svm_vote's labels on the decisions of each cell"""
    n, cells, rows = SCORE_CLASSES, SCORE_CELLS, SCORE_ROWS
    n_pairs = n * (n - 1) // 2
    npp = (n_pairs + 3) // 4 * 4 + 4
    rng = np.random.default_rng([SEED, n])
    dec = rng.choice(DEC_VALUES, (rows, cells * npp + 3))
    wins = []
    for cell in range(cells):
        block = dec[:, cell * npp:cell * npp + n_pairs]
        sweep_rows(block, n, (n - 1, cell, 7))
        block[3] = np.nan
        wins.append(E.vote(block, n))
    truth = np.where(rng.random(rows) < 0.6, wins[1], rng.integers(0, n, rows)).astype(I32)
    truth[:4] = (n - 1, 1, 7, n - 1)
    start = np.array([3, 0, 1000, 77], I32)  # (accumulates on what is there; the slot past the last cell is not a cell)
    correct = Op("correct", start)
    counts = [int((wins[cell] == truth).sum()) for cell in range(cells)]
    assert min(counts) >= 3 and len(set(counts)) > 1
    correct.want[:cells] += np.array(counts, I32)
    correct.windows = [(0, cells)]
    args = (Op("dec", dec), dec.shape[1], rows, n, cells, npp, Op("truth", truth), correct)
    launch(be, "svm_vote_score", *args)
    settle("svm_vote_score", *args)
    for cell in range(cells):
        out = Op("out", sent(U8, rows + 3))
        out.windows = [(0, rows)]
        args = (Op("dec", dec.reshape(-1)[cell * npp:]), dec.shape[1], rows, n, None, None, out, 0)
        launch(be, "svm_vote", *args)
        assert int((out.got[:rows] == truth).sum()) == counts[cell]
        out.want[:rows] = wins[cell]
        settle("svm_vote", *args, tag=f"cell {cell}")
    one = np.zeros((1, 256 * 255 // 2), F32)
    refused = (Op("dec", one), one.shape[1], 1, 256, 1, one.shape[1], Op("truth", np.zeros(1, I32)), Op("correct", start))
    launch(be, "svm_vote_score", *refused, refused=True)
    settle("svm_vote_score", *refused, tag="256 classes")
