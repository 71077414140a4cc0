"""-m gpu: the batch-norm chain of csrc/elementwise.hip -- chunk statistics, their finaliser and the multi-rank merge,
the one-launch short-matrix forms, the fused post-op forward and its two-pass backward -- against the float64
definitions of tests/bn_ref.py, within the bounds DERIVED there (counts of fp32 roundings along the method, times a
margin of 2; tests/test_bn_ref.py shows on the CPU that they hold for an fp32 twin of the method and reject three naive
ones).  No tolerance here comes from what the device produced.

Placement: every output is a window in the middle of a larger tensor whose other elements -- before, behind and in the
pad columns of padded rows -- hold one fixed NaN bit pattern and are compared bit for bit afterwards, so a stray store
is seen and lands inside the allocation.  Inputs sit at element offsets as well (a misaligned base selects the scalar
kernels), and their pad columns hold NaN: a kernel that read them could not meet any bound."""
import collections
import functools

import numpy as np
import pytest

from hypelcnn_amd.backend import Ref
from tests import bn_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS, DECAY, ALPHA = 1e-3, 0.95, 0.18
GUARD_BITS = 0x7FC0BEEF       # a quiet NaN no kernel produces
LEAD_ALIGNED, LEAD_ODD = 64, 61
WORST = collections.defaultdict(lambda: [0.0, 0.0, 0.0])   # (family, quantity) -> [worst error / bound, error, bound]


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    yield HipBackend()
    print("\nworst observed error per family (error / derived bound; the absolute pair at the worst element)")
    for (fam, what), (ratio, err, bound) in sorted(WORST.items()):
        print(f"  bn-chain family {fam} {what:10s} ratio {ratio:8.4f}   error {err:.3e}   bound {bound:.3e}")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _guard(n):
    return np.full(int(n), GUARD_BITS, np.uint32).view(np.float32)


class Win:
    """`data` (or n guard-filled elements) at element offset `lead` of a tensor with `tail` guard elements behind."""

    def __init__(self, hip, data, lead=LEAD_ODD, tail=96):
        data = _guard(data) if isinstance(data, (int, np.integer)) else np.ascontiguousarray(data, np.float32).reshape(-1)
        self.n, self.lead, self.tail = data.size, int(lead), int(tail)
        self.t = hip.upload(np.concatenate([_guard(lead), data, _guard(tail)]))
        self.ref = Ref(self.t, lead)

    def read(self, what="window"):
        full = self.t.cpu().numpy()
        assert np.array_equal(_bits(full[:self.lead]), _bits(_guard(self.lead))), f"{what}: store before the window"
        assert np.array_equal(_bits(full[self.lead + self.n:]), _bits(_guard(self.tail))), f"{what}: store behind it"
        return full[self.lead:self.lead + self.n].copy()

    def mat(self, rows, ld, c, what="matrix"):
        """The live [rows x c] part of a [rows x ld] window; the pad columns must still hold the guard pattern."""
        m = self.read(what).reshape(rows, ld)
        assert np.array_equal(_bits(m[:, c:]), _bits(_guard(rows * (ld - c))).reshape(rows, ld - c)), f"{what}: pad columns"
        return m[:, :c]


def _padded(a, ld):
    """[rows x c] -> flat [rows x ld] with NaN guard pattern in the pad columns."""
    rows, c = a.shape
    out = _guard(rows * ld).reshape(rows, ld).copy()
    out[:, :c] = a
    return out


def _in(hip, a, ld, lead):
    """An input matrix window; one row of guard behind the last row's pad."""
    return Win(hip, _padded(np.asarray(a, np.float32), ld), lead, tail=2 * ld + 64)


def _out(hip, rows, ld, lead):
    return Win(hip, rows * ld, lead, tail=2 * ld + 64)


def _within(got, want, bound, fam, what):
    """|got - want| <= bound elementwise (axis -1 = columns, families per column); records the worst ratio."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    err = np.abs(got - want)
    g2, e2, b2 = (np.broadcast_to(a, np.broadcast(got, want, bound).shape).reshape(-1, got.shape[-1]) for a in (got, err, bound))
    for f in sorted(set(fam)):
        cols = np.flatnonzero(fam == f)
        e, b = e2[:, cols], b2[:, cols]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(e == 0, 0.0, e / b)
        i = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.size else None
        if i is not None and np.isfinite(ratio[i]) and ratio[i] > WORST[(f, what)][0]:
            WORST[(f, what)] = [float(ratio[i]), float(e[i]), float(b[i])]
    bad = ~(err <= bound)
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements outside the derived bound; worst error / bound "
                           f"{np.nanmax(np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0))):.3f}, "
                           f"families {sorted(set(np.broadcast_to(fam, got.shape)[bad]))}")


def _v4(ref, c, ld):
    """launch_col_stats / launch_bwd_reduce / the elementwise launchers take the float4 form iff c and the leading
    dimension are multiples of 4 and the base is 16-byte aligned."""
    return c % 4 == 0 and ld % 4 == 0 and ref.ptr() % 16 == 0


# ======================================================================================= statistics + finaliser
# (rows, c, chunk_rows, ld, lead, form the case is meant to reach)
STATS_CASES = [(4097, 20, 16, 20, LEAD_ALIGNED, "v4"),        # 257 chunks: second sweep, one-row last chunk
               (4097, 19, 16, 23, LEAD_ODD, "scalar"),        # padded rows
               (8200, 68, 16, 68, LEAD_ALIGNED, "v4"),        # 513 chunks: third sweep; > 64 columns, 16-channel blocks
               (17, 130, 16, 132, LEAD_ALIGNED, "scalar"),    # two chunks; 130 = 8 * 16 + 2
               (1, 5, 16, 5, LEAD_ODD, "scalar"),             # one row: Bessel branch n == 1
               (257, 16, 256, 16, LEAD_ALIGNED + 1, "scalar")]  # c % 4 == 0 but the base is off by one element


def _stats_launch(hip, x, rows, c, chunk, ld, lead, mm0, mv0):
    nch = (rows + chunk - 1) // chunk
    xin = _in(hip, x, ld, lead)
    part, mean, rstd = Win(hip, nch * 2 * c), Win(hip, c), Win(hip, c)
    mm, mv = (None, None) if mm0 is None else (Win(hip, mm0), Win(hip, mv0))
    hip.call("col_stats_partial", xin.ref, ld, rows, c, chunk, part.ref)
    hip.call("bn_finalize", part.ref, nch, chunk, rows, c, EPS, mean.ref, rstd.ref, None if mm is None else mm.ref,
             None if mv is None else mv.ref, DECAY)
    hip.synchronize()
    out = {"part": part.read("partials").reshape(nch, 2, c), "mean": mean.read("mean"), "rstd": rstd.read("rstd")}
    if mm is not None:
        out["mm"], out["mv"] = mm.read("moving_mean"), mv.read("moving_var")
    xin.read("input")
    return out, xin


@pytest.mark.parametrize("rows,c,chunk,ld,lead,form", STATS_CASES)
def test_statistics_and_finaliser_within_the_derived_bounds(hip, rows, c, chunk, ld, lead, form):
    x, fam = R.family_matrix(rows, c, chunk, seed=rows * 1000 + c)
    rng = np.random.default_rng(rows + c)
    mm0, mv0 = rng.standard_normal(c).astype(np.float32), (rng.random(c) + 0.5).astype(np.float32)
    got, xin = _stats_launch(hip, x, rows, c, chunk, ld, lead, mm0, mv0)
    assert _v4(xin.ref, c, ld) == (form == "v4"), "the case reaches another kernel form than it is meant to"
    sb = R.stats_bounds(x, chunk, form, EPS, DECAY)
    mk, qk = R.partials_def(x, chunk)
    mean, m2, _ = R.stats_def(x)
    fin = R.finish_def(mean, m2, rows, EPS, mm0, mv0, DECAY)
    e_mm, e_mv = R.moving_bounds(sb, fin["mm"], fin["mv"])
    _within(got["part"][:, 0], mk, sb["part_mean"], fam, "chunk mean")
    _within(got["part"][:, 1], qk, sb["part_m2"], fam, "chunk M2")
    _within(got["mean"], fin["mean"], sb["mean"], fam, "mean")
    _within(got["rstd"], fin["rstd"], sb["rstd"], fam, "rstd")
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(got["rstd"] - fin["rstd"]) / fin["rstd"]
    for f in sorted(set(fam)):
        print(f"family {f}: rstd relative error {rel[fam == f].max():.3e}, bound {(sb['rstd'] / fin['rstd'])[fam == f].max():.3e}")
    _within(got["mm"], fin["mm"], e_mm, fam, "moving mean")
    _within(got["mv"], fin["mv"], e_mv, fam, "moving var")
    # b: constant column -- d == 0 everywhere, so nothing rounds
    b = fam == "b"
    assert np.array_equal(_bits(got["part"][:, 0, b]), _bits(np.full((mk.shape[0], int(b.sum())), 3.25)))
    assert np.array_equal(_bits(got["part"][:, 1, b]), np.zeros((mk.shape[0], int(b.sum())), np.uint32)), "M2 is +0"
    assert np.array_equal(_bits(got["mean"][b]), _bits(np.full(int(b.sum()), 3.25)))
    assert np.array_equal(_bits(got["rstd"][b]), _bits(np.full(int(b.sum()), F32(1.0 / np.sqrt(float(F32(EPS)))))))
    # e: +-1 alternating -- every fp32 sum is a small integer
    e = fam == "e"
    if e.any() and R.sums_exact(rows, chunk):
        assert np.array_equal(_bits(got["part"][:, 0, e]), _bits(mk[:, e].astype(np.float32)))
        assert np.array_equal(_bits(got["part"][:, 1, e]), _bits(qk[:, e].astype(np.float32)))
        assert np.array_equal(_bits(got["mean"][e]), _bits(fin["mean"][e].astype(np.float32)))
        assert np.array_equal(_bits(got["rstd"][e]), _bits(fin["rstd"][e].astype(np.float32)))
    # moving statistics NULL: mean / rstd do not depend on them
    again, _ = _stats_launch(hip, x, rows, c, chunk, ld, lead, None, None)
    for k in ("part", "mean", "rstd"):
        assert np.array_equal(_bits(again[k]), _bits(got[k])), f"{k} differs without moving statistics"
    # g: one NaN and one +Inf stay in their columns
    jn, ji = 0, c - 1
    xg = x.copy()
    xg[rows // 2, jn], xg[rows // 3, ji] = np.nan, np.inf
    bad, _ = _stats_launch(hip, xg, rows, c, chunk, ld, lead, mm0, mv0)
    for j, r in ((jn, rows // 2), (ji, rows // 3)):
        assert not np.isfinite(bad["mean"][j]) and not np.isfinite(bad["rstd"][j]), f"column {j}: {bad['mean'][j]}, {bad['rstd'][j]}"
        assert not np.isfinite(bad["part"][r // chunk, 0, j])
        assert not np.isfinite(bad["mm"][j]) and not np.isfinite(bad["mv"][j])
        assert np.isnan(bad["part"][r // chunk, 1, j]), "a chunk with a NaN or an Inf has no M2 (Inf - Inf)"
    rest = np.ones(c, bool)
    rest[[jn, ji]] = False
    for k in ("mean", "rstd", "mm", "mv"):
        assert np.array_equal(_bits(bad[k][rest]), _bits(got[k][rest])), f"{k}: a non-finite column leaked"
    assert np.array_equal(_bits(bad["part"][:, :, rest]), _bits(got["part"][:, :, rest]))


# ============================================================================================ multi-rank merge
RANK_ROWS = {1: [4129], 3: [4129, 1, 300], 8: [4129, 1, 17, 33, 250, 64, 5, 1000]}   # 4129 = 258 * 16 + 1: 259 chunks


@pytest.mark.parametrize("world", [1, 3, 8])
def test_rank_merge_is_the_statistics_of_the_concatenated_rows(hip, world):
    c, chunk, form = 24, 16, "v4"
    xs, fam = [], None
    for r, rows in enumerate(RANK_ROWS[world]):
        x, fam = R.family_matrix(rows, c, chunk, seed=100 * world + r)
        xs.append(x)
    rec = 2 * c + 1
    allrec = Win(hip, world * rec)
    e_rm, e_rq, r_mean = [], [], []
    for r, x in enumerate(xs):
        rows = x.shape[0]
        nch = (rows + chunk - 1) // chunk
        xin, part = _in(hip, x, c, LEAD_ALIGNED), Win(hip, nch * 2 * c)
        assert _v4(xin.ref, c, c)
        hip.call("col_stats_partial", xin.ref, c, rows, c, chunk, part.ref)
        hip.call("bn_merge_partials", part.ref, nch, chunk, rows, c, allrec.ref + r * rec)
        hip.synchronize()
        part.read("partials")
        mk, _ = R.partials_def(x, chunk)
        em, eq = R.partial_bounds(x, chunk, form)
        e_mean, e_m2 = R.merge_bounds(R.chunk_sizes(rows, chunk), mk, em, eq)
        mean_r, m2_r, _ = R.stats_def(x)
        e_rm.append(e_mean + R.rnd(mean_r))       # the record is stored as float32
        e_rq.append(e_m2 + R.rnd(m2_r))
        r_mean.append(mean_r)
    got = allrec.read("records").reshape(world, rec)
    k = R.MARGIN * R.SLACK
    for r, x in enumerate(xs):
        mean_r, m2_r, _ = R.stats_def(x)
        assert _bits(got[r, 2 * c:])[0] == _bits(np.array([x.shape[0]], np.float32))[0], "out[2c] holds the row count"
        _within(got[r, :c], mean_r, k * e_rm[r], fam, "rank mean")
        _within(got[r, c:2 * c], m2_r, k * e_rq[r], fam, "rank M2")
    rng = np.random.default_rng(world)
    mm0, mv0 = rng.standard_normal(c).astype(np.float32), (rng.random(c) + 0.5).astype(np.float32)
    mean, rstd, mm, mv = Win(hip, c), Win(hip, c), Win(hip, mm0), Win(hip, mv0)
    hip.call("bn_finalize_ranks", allrec.ref, world, c, EPS, mean.ref, rstd.ref, mm.ref, mv.ref, DECAY)
    hip.synchronize()
    xall = np.concatenate(xs)
    n = xall.shape[0]
    mean_d, m2_d, _ = R.stats_def(xall)
    fin = R.finish_def(mean_d, m2_d, n, EPS, mm0, mv0, DECAY)
    n_r = [x.shape[0] for x in xs]
    e_mean, e_m2 = R.merge_bounds(n_r, np.array(r_mean), np.array(e_rm), np.array(e_rq))
    dec = float(F32(DECAY))
    _within(mean.read(), fin["mean"], k * (e_mean + R.rnd(mean_d)), fam, "merged mean")
    _within(rstd.read(), fin["rstd"], k * R.rstd_bound(m2_d, e_m2, n, EPS), fam, "merged rstd")
    _within(mm.read(), fin["mm"], k * ((1 - dec) * e_mean + R.rnd(fin["mm"])), fam, "merged mm")
    _within(mv.read(), fin["mv"], k * ((1 - dec) * e_m2 / (n - 1) + R.rnd(fin["mv"])), fam, "merged mv")
    b = fam == "b"
    assert np.array_equal(_bits(mean.read()[b]), _bits(np.full(int(b.sum()), 3.25)))
    assert np.array_equal(_bits(rstd.read()[b]), _bits(np.full(int(b.sum()), F32(1.0 / np.sqrt(float(F32(EPS)))))))


# ========================================================================================== short-matrix forms
SMALL_ROWS = [1024, 1023, 993, 33, 32, 31, 1]
SMALL_C = [1, 31, 32, 33, 65]
ACTS = [R.ACT_NONE, R.ACT_LRELU, R.ACT_RELU, R.ACT_SIGMOID, R.ACT_TANH]


@functools.lru_cache(maxsize=None)
def _small_inputs(rows, c):
    rng = np.random.default_rng(rows * 100 + c)
    y, fam = R.family_matrix(rows, c, 256, seed=rows * 100 + c, fams="abcde")
    d = {"y": y, "dz": rng.standard_normal((rows, c)).astype(np.float32),
         "mask": ((rng.random((rows, c)) < 0.7) / F32(0.7)).astype(np.float32),
         "beta": rng.standard_normal(c).astype(np.float32), "mm0": rng.standard_normal(c).astype(np.float32),
         "mv0": (rng.random(c) + 0.5).astype(np.float32), "dp0": rng.standard_normal(c).astype(np.float32)}
    for a in d.values():
        a.setflags(write=False)
    return d, fam


@pytest.mark.parametrize("c", SMALL_C)
@pytest.mark.parametrize("rows", SMALL_ROWS)
def test_short_matrix_forms_reject_rows_and_columns_outside(hip, rows, c):
    """bn_act_small_fwd / _bwd for every activation, with and without mask, dparam accumulating and not; and the wide
    chain on the same input.  Row counts: the FULL template (1024), the first ragged count (1023), one live row lane in
    the last register row (993), around the 32-lane boundary, and 1; column counts around the 32-column block."""
    d, fam = _small_inputs(rows, c)
    ld = c + 3
    y, dz, mask, beta = d["y"], d["dz"], d["mask"], d["beta"]
    yin, dzin, mkin = _in(hip, y, ld, 1), _in(hip, dz, ld, 3), _in(hip, mask, ld, 2)
    bt = Win(hip, beta, 1)
    sb = R.stats_bounds(y, rows, "small", EPS, DECAY)
    mean_d, m2_d, _ = R.stats_def(y)
    fin = R.finish_def(mean_d, m2_d, rows, EPS, d["mm0"], d["mv0"], DECAY)
    e_mm, e_mv = R.moving_bounds(sb, fin["mm"], fin["mv"])
    first = None
    for act in ACTS:
        for use_mask in (False, True):
            m = mask if use_mask else None
            mean, rstd, mm, mv = Win(hip, c), Win(hip, c), Win(hip, d["mm0"]), Win(hip, d["mv0"])
            z = _out(hip, rows, ld, LEAD_ODD)
            hip.call("bn_act_small_fwd", yin.ref, ld, rows, c, EPS, bt.ref, act, ALPHA, mkin.ref if use_mask else None,
                     ld, mean.ref, rstd.ref, mm.ref, mv.ref, DECAY, z.ref, ld)
            hip.synchronize()
            mu, rs = mean.read("mean"), rstd.read("rstd")
            if first is None:
                first = (mu, rs)
                _within(mu, fin["mean"], sb["mean"], fam, "small mean")
                _within(rs, fin["rstd"], sb["rstd"], fam, "small rstd")
                _within(mm.read("mm"), fin["mm"], e_mm, fam, "small mm")
                _within(mv.read("mv"), fin["mv"], e_mv, fam, "small mv")
                b = fam == "b"
                assert np.array_equal(_bits(mu[b]), _bits(np.full(int(b.sum()), 3.25)))
                assert np.array_equal(_bits(rs[b]), _bits(np.full(int(b.sum()), F32(1.0 / np.sqrt(float(F32(EPS)))))))
            else:
                assert np.array_equal(_bits(mu), _bits(first[0])) and np.array_equal(_bits(rs), _bits(first[1]))
                mm.read("mm"), mv.read("mv")
            zz = z.mat(rows, ld, c, f"z act {act} mask {use_mask}")
            if act in (R.ACT_NONE, R.ACT_LRELU, R.ACT_RELU) and not use_mask:
                assert np.array_equal(_bits(zz), _bits(R.fwd_f32(y, mu, rs, beta, act, ALPHA))), f"z act {act}: not the separately rounded pre"
            else:
                _within(zz, R.fwd_def(y, mu, rs, beta, act, ALPHA, m), R.fwd_bound(y, mu, rs, beta, act, ALPHA, m), fam, "small z")
            bb = R.bwd_bounds(dz, y, mu, rs, beta, act, ALPHA, m, rows, "small")
            for acc in (0, 1):
                dy, dp = _out(hip, rows, ld, LEAD_ODD), Win(hip, d["dp0"])
                hip.call("bn_act_small_bwd", dzin.ref, ld, yin.ref, ld, rows, c, mean.ref, rstd.ref, bt.ref, act, ALPHA,
                         mkin.ref if use_mask else None, ld, dy.ref, ld, dp.ref, acc)
                hip.synchronize()
                _within(dy.mat(rows, ld, c, f"dy act {act}"), bb["def"]["dy"], bb["dy"], fam, "small dy")
                want = bb["def"]["s0"] + (d["dp0"] if acc else 0.0)
                _within(dp.read("dparam"), want, bb["s0"] + (R.MARGIN * R.rnd(want) if acc else 0.0), fam, "small dbeta")
            mean.read("mean"), rstd.read("rstd")
    for w in (yin, dzin, mkin, bt):
        w.read("input")
    # the wide chain on the same input meets the same definition, so the two paths agree within the sum of their bounds
    chunk = 256
    wide, xin = _stats_launch(hip, y, rows, c, chunk, ld, LEAD_ODD, d["mm0"], d["mv0"])
    assert not _v4(xin.ref, c, ld)
    wb = R.stats_bounds(y, chunk, "scalar", EPS, DECAY)
    _within(wide["mean"], fin["mean"], wb["mean"], fam, "mean")
    _within(wide["rstd"], fin["rstd"], wb["rstd"], fam, "rstd")
    assert (np.abs(wide["mean"].astype(np.float64) - first[0]) <= wb["mean"] + sb["mean"]).all()
    assert (np.abs(wide["rstd"].astype(np.float64) - first[1]) <= wb["rstd"] + sb["rstd"]).all()


# ========================================================================== post-op forward and two-pass backward
# (rows, c, chunk_rows): (5, 1028) is 257 column vectors, past the 256-thread cap of ew_shape; (4097, 20) and
# (8200, 68) with 16-row chunks take the backward finaliser through its second and third sweep
POST_CASES = [(1, 1, 256), (3, 257, 256), (5, 1028, 256), (4097, 20, 16), (8200, 68, 16)]


@functools.lru_cache(maxsize=None)
def _post_inputs(rows, c, chunk):
    rng = np.random.default_rng(rows * 7 + c)
    y, fam = R.family_matrix(rows, c, chunk, seed=rows * 7 + c, fams="abcde")
    mean, m2, _ = R.stats_def(y)
    d = {"y": y, "dz": rng.standard_normal((rows, c)).astype(np.float32),
         "mask": ((rng.random((rows, c)) < 0.7) / F32(0.7)).astype(np.float32),
         "r1": rng.standard_normal((rows, c)).astype(np.float32), "r2": rng.standard_normal((rows, c)).astype(np.float32),
         "beta": rng.standard_normal(c).astype(np.float32), "dp0": rng.standard_normal(c).astype(np.float32),
         # the batch's own statistics, rounded to float32 as the finaliser stores them
         "mean": mean.astype(np.float32), "rstd": R.finish_def(mean, m2, rows, EPS)["rstd"].astype(np.float32),
         "gsums": (rng.standard_normal((2, c)) * 10).astype(np.float32)}
    for a in d.values():
        a.setflags(write=False)
    return d, fam


@pytest.mark.parametrize("rows,c,chunk", POST_CASES)
def test_post_op_forward_and_backward_against_the_definition(hip, rows, c, chunk):
    d, fam = _post_inputs(rows, c, chunk)
    v4 = c % 4 == 0
    ld = c + 4 if v4 else c + 3
    lead = LEAD_ALIGNED if v4 else LEAD_ODD
    form = "v4" if v4 else "scalar"
    y, dz, mask, beta, mu, rs = d["y"], d["dz"], d["mask"], d["beta"], d["mean"], d["rstd"]
    yin, dzin, mkin = _in(hip, y, ld, lead), _in(hip, dz, ld, lead), _in(hip, mask, ld, lead)
    r1, r2 = _in(hip, d["r1"], ld, lead), _in(hip, d["r2"], ld, lead)
    mt, rt, bt = Win(hip, mu, 1), Win(hip, rs, 3), Win(hip, beta, 2)   # parameters at arbitrary element offsets
    assert _v4(yin.ref, c, ld) == v4
    nch = (rows + chunk - 1) // chunk
    for act in ACTS:
        # -- forward, bare: the contract(off) promise, bit for bit
        if act in (R.ACT_NONE, R.ACT_LRELU, R.ACT_RELU):
            z = _out(hip, rows, ld, lead)
            hip.call("bn_act_fwd", yin.ref, ld, rows, c, mt.ref, rt.ref, bt.ref, act, ALPHA, None, 0, None, 0, None,
                     None, 0, None, z.ref, ld)
            hip.synchronize()
            assert np.array_equal(_bits(z.mat(rows, ld, c, "z")), _bits(R.fwd_f32(y, mu, rs, beta, act, ALPHA))), f"act {act}"
        # -- forward with mask and two residuals: a few U per operation (bn_ref.fwd_bound)
        z = _out(hip, rows, ld, lead)
        hip.call("bn_act_fwd", yin.ref, ld, rows, c, mt.ref, rt.ref, bt.ref, act, ALPHA, mkin.ref, ld, r1.ref, ld, None,
                 r2.ref, ld, None, z.ref, ld)
        hip.synchronize()
        res = (d["r1"], d["r2"])
        _within(z.mat(rows, ld, c, "z"), R.fwd_def(y, mu, rs, beta, act, ALPHA, mask, res),
                R.fwd_bound(y, mu, rs, beta, act, ALPHA, mask, res), fam, "z")
        # -- backward: reduce -> finalise -> apply
        for use_mask in (False, True):
            m = mask if use_mask else None
            bb = R.bwd_bounds(dz, y, mu, rs, beta, act, ALPHA, m, chunk, form)
            df = bb["def"]
            part, sums, dy = Win(hip, nch * 2 * c), Win(hip, 2 * c), _out(hip, rows, ld, lead)
            hip.call("bn_act_bwd_reduce", dzin.ref, ld, yin.ref, ld, rows, c, mt.ref, rt.ref, bt.ref, act, ALPHA,
                     mkin.ref if use_mask else None, ld, chunk, part.ref)
            for acc in (0, 1):
                dp = Win(hip, d["dp0"])
                hip.call("bwd_reduce_finalize", part.ref, nch, c, sums.ref, dp.ref, acc)
                hip.synchronize()
                want = df["s0"] + (d["dp0"] if acc else 0.0)
                _within(dp.read("dparam"), want, bb["s0"] + (R.MARGIN * R.rnd(want) if acc else 0.0), fam, "dbeta")
            hip.call("bwd_reduce_finalize", part.ref, nch, c, sums.ref, None, 0)
            hip.call("bn_act_bwd_apply", dzin.ref, ld, yin.ref, ld, rows, c, mt.ref, rt.ref, bt.ref, act, ALPHA,
                     mkin.ref if use_mask else None, ld, sums.ref, dy.ref, ld)
            hip.synchronize()
            part.read("partials")
            s = sums.read("sums").reshape(2, c)
            _within(s[0], df["s0"], bb["s0"], fam, "s0")
            _within(s[1], df["s1"], bb["s1"], fam, "s1")
            dyv = dy.mat(rows, ld, c, "dy")
            _within(dyv, df["dy"], bb["dy"], fam, "dy")
            # Property: with the batch's own statistics the column sums of dy and of dy * xhat vanish.  In exact
            # arithmetic sum_r dy = -rstd (s1 / N) sum_r xhat and sum_r dy xhat = rstd (s1 (1 - sum xhat^2 / N) -
            # (s0 / N) sum xhat): sum xhat is N (mean - fl(mean)) rstd and 1 - sum xhat^2 / N is eps rstd^2 (plus the
            # rounding of rstd), both evaluated below in float64 from the data.  The device adds at most its error
            # on every dy (bb["dy"], derived in bn_ref.bwd_bounds), times |xhat| in the second sum.
            xh = df["xhat"]
            n = float(rows)
            r0 = -rs.astype(np.float64) * (df["s1"] / n) * xh.sum(0)
            r1_ = rs.astype(np.float64) * (df["s1"] * (1 - (xh * xh).sum(0) / n) - (df["s0"] / n) * xh.sum(0))
            tiny = 1e-12 * (np.abs(df["dy"]).sum(0) + 1e-300)     # the float64 evaluation of the residuals themselves
            assert (np.abs(dyv.astype(np.float64).sum(0)) <= np.abs(r0) + bb["dy"].sum(0) + tiny).all(), "sum dy"
            assert (np.abs((dyv * xh).sum(0)) <= np.abs(r1_) + (bb["dy"] * np.abs(xh)).sum(0) + tiny * (1 + np.abs(xh).max(0))).all(), "sum dy xhat"
        # -- the global-batch form: sums of a batch of stat_rows > rows rows are inputs
        stat_rows = 3 * rows + 5
        gs, dy = Win(hip, d["gsums"], 3), _out(hip, rows, ld, lead)
        hip.call("bn_act_bwd_apply_global", dzin.ref, ld, yin.ref, ld, rows, c, mt.ref, rt.ref, bt.ref, act, ALPHA,
                 mkin.ref, ld, gs.ref, stat_rows, dy.ref, ld)
        hip.synchronize()
        bg = R.bwd_bounds(dz, y, mu, rs, beta, act, ALPHA, mask, chunk, form, stat_rows, d["gsums"])
        _within(dy.mat(rows, ld, c, "dy global"), bg["def"]["dy"], bg["dy"], fam, "dy global")
        gs.read("sums")
    for w in (yin, dzin, mkin, r1, r2, mt, rt, bt):
        w.read("input")


# ==================================================================================================== the kink
@pytest.mark.parametrize("act,slope0", [(R.ACT_LRELU, F32(ALPHA)), (R.ACT_RELU, F32(0.0))])
def test_forward_and_backward_take_the_same_branch_at_the_kink(hip, act, slope0):
    """Columns with y == mean (so xhat == 0 and pre == beta exactly) and beta in {0, +1e-30, -1e-30}: the forward value
    and the backward slope come from the same branch -- pre > 0: (pre, 1); pre <= 0: (pre * slope0, slope0), with value
    0 at pre == 0 -- on the wide path (slope read from dy with zero sums and dz == 1: dy = fl(rstd * slope)) and on the
    short-matrix path (slope read from dparam with dz == 1 in one row: dparam = slope)."""
    rows, c = 8, 6
    beta = np.array([0.0, 1e-30, -1e-30, 0.0, 1e-30, -1e-30], np.float32)
    y = np.full((rows, c), 3.25, np.float32)
    rstd = F32(1.0 / np.sqrt(float(F32(EPS))))           # what both paths compute for a constant column
    pos = beta > 0
    want_z = np.where(pos, beta, (beta * slope0).astype(np.float32)).astype(np.float32)
    want_slope = np.where(pos, F32(1.0), slope0).astype(np.float32)
    assert want_z[0] == 0 and want_z[1] == F32(1e-30) and want_slope[0] == slope0
    ld = c + 3
    yin, bt = _in(hip, y, ld, 1), Win(hip, beta, 1)
    # wide path
    mt, rt = Win(hip, np.full(c, 3.25, np.float32), 1), Win(hip, np.full(c, rstd, np.float32), 1)
    z, dy = _out(hip, rows, ld, LEAD_ODD), _out(hip, rows, ld, LEAD_ODD)
    dzin, sums = _in(hip, np.ones((rows, c), np.float32), ld, 1), Win(hip, np.zeros(2 * c, np.float32))
    hip.call("bn_act_fwd", yin.ref, ld, rows, c, mt.ref, rt.ref, bt.ref, act, ALPHA, None, 0, None, 0, None, None, 0,
             None, z.ref, ld)
    hip.call("bn_act_bwd_apply", dzin.ref, ld, yin.ref, ld, rows, c, mt.ref, rt.ref, bt.ref, act, ALPHA, None, 0,
             sums.ref, dy.ref, ld)
    hip.synchronize()
    zz, dd = z.mat(rows, ld, c, "z"), dy.mat(rows, ld, c, "dy")
    assert (zz == want_z).all() and np.array_equal(_bits(zz[:, pos]), _bits(np.broadcast_to(want_z[pos], (rows, int(pos.sum())))))
    assert np.array_equal(_bits(dd), _bits(np.broadcast_to((rstd * want_slope).astype(np.float32), (rows, c))))
    assert ((zz > 0) == (dd == rstd)).all(), "forward and backward disagree about the branch"
    # short-matrix path: the kernel finds mean == 3.25 and the same rstd itself
    mean, rs, zs = Win(hip, c), Win(hip, c), _out(hip, rows, ld, LEAD_ODD)
    hip.call("bn_act_small_fwd", yin.ref, ld, rows, c, EPS, bt.ref, act, ALPHA, None, 0, mean.ref, rs.ref, None, None,
             DECAY, zs.ref, ld)
    one_row = np.zeros((rows, c), np.float32)
    one_row[0] = 1.0
    dz1, dys, dp = _in(hip, one_row, ld, 1), _out(hip, rows, ld, LEAD_ODD), Win(hip, c)
    hip.call("bn_act_small_bwd", dz1.ref, ld, yin.ref, ld, rows, c, mean.ref, rs.ref, bt.ref, act, ALPHA, None, 0,
             dys.ref, ld, dp.ref, 0)
    hip.synchronize()
    assert np.array_equal(_bits(mean.read()), _bits(np.full(c, 3.25))) and np.array_equal(_bits(rs.read()), _bits(np.full(c, rstd)))
    zz = zs.mat(rows, ld, c, "z small")
    assert (zz == want_z).all() and np.array_equal(_bits(zz[:, pos]), _bits(np.broadcast_to(want_z[pos], (rows, int(pos.sum())))))
    slope = dp.read("dparam")
    assert np.array_equal(_bits(slope), _bits(want_slope)), f"slopes {slope}"
    assert ((zz[0] > 0) == (slope == 1)).all()
    dys.mat(rows, ld, c, "dy small")
