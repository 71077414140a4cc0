"""TEST INFRASTRUCTURE shared by tests/test_gpu_head_kernels.py (the HIP kernels, through the C-ABI) and
tests/test_head_kernel_cases_emu.py (the executable spec alone): the classifier's layout, LRN, loss-head, metric, gather
and copy kernels -- case tables, operand layouts, references and checks.  Every `run_*` function takes a
parity_util.Both or parity_util.SpecOnly and checks what that object's device side holds after the launches.

Operands.  Every row operand is a window of a sentinel-filled allocation (`Win`, a parity_util.Arena with a lead): its own
leading dimension and an odd column offset, so that its base is only 4-byte aligned ("odd"), or a leading dimension that
is a multiple of 4 at a 16-byte base ("aligned"), so that both the float4 and the scalar dispatch of a kernel run.  After
each launch everything outside the output window must still hold the sentinel's bits.

References.  float64 NumPy written from the operation's definition (include/hypel.h), not from a kernel's index
arithmetic.  Pure data movement (layout, gathers, augmentation, copies) is compared bit for bit against a NumPy / torch
composition (transpose, slicing, rot90, flip).  Everything else is held to a bound derived in the docstring of its
function as a count of fp32 roundings, in units of U = 2^-24 of the magnitude named there; the only measured figures are
the device powf's ulp errors (tools/exp/probe/libm_ulp_probe.hip), handed in by the test files.  Nothing in a bound comes
from a kernel's output.

Yardstick.  Next to each bounded quantity the same formula is evaluated in plain float32 NumPy (window sums term by term,
np.power on float32, np.sum with dtype float32): it must lie within the same bound of the float64 reference -- a bound
that plain fp32 cannot meet is wrong.  `Report` collects, per label, the largest error / bound ratio of the device side
and of the yardstick; the CPU test asserts the yardstick's.

Overflow is outside every contract here: |x| <= 1e18 for the LRN kernels (x^2 stays finite in fp32), |a - b| <= 1e15 for
the squared error."""
import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import COPY_BLOCK_DTYPE, HypelError
from tests.parity_util import SENT, Arena, assert_same_bits, bits

U = 2.0 ** -24            # unit roundoff of fp32: one rounding moves a value by at most U * |value| (half an ulp)
TINY = 2.0 ** -150        # half the spacing of the fp32 subnormals: the absolute floor of one rounding
SLACK = 1.0 + 1e-6        # second-order terms (U^2) and the float64 reference's own rounding (2^-53)
F32 = np.float32
MSE_PARTIALS = 1024       # include/hypel.h HYPEL_MSE_PARTIALS; also the "ws >= 1024 floats" of hypel_mse / hypel_sum_f32
RED_BLOCKS = 1024         # most blocks of the two-stage reductions (one partial each: the 1024 floats of ws)
ISENT = np.int32(-77777)  # the canary of the int32 outputs
BSENT = np.uint8(0xA5)    # ... and of the bytes round a raster


def roundup4(v):
    return (int(v) + 3) // 4 * 4


class Win(Arena):
    """parity_util.Arena with `lead` further sentinel floats in front: a window whose leading dimension equals its
    width can still start at a base that is only 4-byte aligned.  The guard is 16 rows of at least 16 and at most 256
    floats (an Arena's 16 * ld would be 64 MB round the half-million-element cases; 256 floats cover the 192 columns a
    pass of nhwc_to_pnc_kernel may look ahead)."""

    def __init__(self, n, width, ld=None, col=0, data=None, lead=0):
        ld = width if ld is None else ld
        assert 0 <= col and col + width <= ld
        self.n, self.width, self.ld, self.col = int(n), int(width), int(ld), int(col)
        self.guard = 16 * min(max(self.ld, 16), 256) + int(lead)
        self.off = self.guard + self.col
        self.buf = np.full(2 * self.guard + self.n * self.ld, SENT, np.float32)
        if data is not None:
            self.window(self.buf)[...] = np.asarray(data, np.float32).reshape(self.n, self.width)

    @property
    def aligned16(self):
        return self.off % 4 == 0


def win(n, width, layout, data=None):
    """'odd': ld = width + 3, column 1 (base 4-byte aligned only); 'aligned': ld = the next multiple of 4 above the
    width, column 0 (16-byte base); 'tight': ld = width at a 16-byte base; 'tight+1': the same behind one more float"""
    if layout == "odd":
        return Win(n, width, width + 3, 1, data)
    if layout == "aligned":
        return Win(n, width, roundup4(width + 1), 0, data)
    return Win(n, width, width, 0, data, lead=1 if layout == "tight+1" else 0)


def dev(b, name):
    """what the device side holds under `name` (the spec's own array under SpecOnly)"""
    return b.h[name].cpu().numpy()


class IntGuard:
    """an int32 / uint8 output of `size` elements between `g` canaries"""

    def __init__(self, size, dtype=np.int32, init=None, g=7):
        self.size, self.g, self.sent = int(size), g, ISENT if dtype == np.int32 else BSENT
        self.buf = np.full(size + 2 * g, self.sent, dtype)
        if init is not None:
            self.buf[g:g + size] = init
        self.off = g

    def payload(self, flat):
        return np.asarray(flat)[self.g:self.g + self.size]

    def check(self, flat, name):
        flat = np.asarray(flat)
        assert (flat[:self.g] == self.sent).all() and (flat[self.g + self.size:] == self.sent).all(), \
            f"{name}: written outside its {self.size} elements"


class Report(dict):
    """label -> [largest device error / bound, largest yardstick error / bound]"""

    def note(self, label, device, yard):
        cur = self.setdefault(label, [0.0, 0.0])
        cur[0], cur[1] = max(cur[0], device), max(cur[1], yard)

    def worst_yardstick(self):
        return max(self.items(), key=lambda kv: kv[1][1]) if self else ("", [0.0, 0.0])

    def lines(self):
        return [f"{k}: device {v[0]:.3f} of its bound, fp32 yardstick {v[1]:.3f}" for k, v in sorted(self.items())]


def ratio(got, ref, bound):
    """largest |got - ref| / bound; an element whose bound is 0 must be exact (else inf).  `got` must be finite."""
    got, ref, bound = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, np.broadcast_to(bound, np.shape(ref))))
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return np.inf
    err = np.abs(got - ref)
    pos = bound > 0
    r = np.where(pos, err / np.where(pos, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def hold(rep, label, got, ref, bound, yard, where=""):
    """the device side within the derived bound; device and yardstick ratios go into the report (the CPU test asserts
    the yardstick's, so that a device failure and a wrong bound are told apart)"""
    rd, ry = ratio(got, ref, bound), ratio(yard, ref, bound)
    rep.note(label, rd, ry)
    assert rd <= 1.0, f"{label} {where}: error is {rd:.3f} of the derived bound (fp32 yardstick: {ry:.3f})"


# ======================================================================================================= 1. layout
LAYOUT_C = [1, 63, 64, 65, 145, 190, 192, 193, 360]  # 190 with ld = 193 straddles the 192-column pass
LAYOUT_NP = [(1, 1), (1, 3), (3, 1), (2, 2), (1, 5), (5, 1), (17, 1), (1, 17)]  # p * n of {1, 3, 4, 5, 17}: 4 rows a wave
LAYOUT_BIG = (31, 47, 360)  # n * p * c = 524 520 > 2048 * 256: a thread of pnc_to_nhwc_kernel takes a second trip


def layout_lds(c):
    return sorted({c, c + 1, c + 3, roundup4(c + 1)})


def run_layout(b, n, p, c, ld, lead):
    """hypel_nhwc_to_pnc: data columns bit exact against x.transpose(1, 0, 2), pad columns [c, ld) exactly +0, nothing
    outside the p * n rows of ld floats.  hypel_pnc_to_nhwc from a padded input whose pad columns hold sentinels: bit
    exact; and from the first kernel's own output: the round trip is the identity.  x itself lies inside sentinels, so
    a pad column filled from whatever follows a row's c floats is not +0.  (The grid clamp of hypel_nhwc_to_pnc -- more
    than 65536 * 4 blocks of 16 rows -- needs more than 4 M rows: out of reach at test size, not tested.)"""
    rng = np.random.default_rng(1000 * c + 10 * ld + n * p)
    x = rng.standard_normal((n, p, c)).astype(F32)
    x.reshape(-1)[::7] = F32(-0.0)  # a sign bit a float comparison would not see
    want = x.transpose(1, 0, 2).reshape(p * n, c)
    xin = Win(1, n * p * c, data=x, lead=lead)
    out = Win(p * n, ld, lead=lead)
    b.arr("x", xin.buf), b.arr("out", out.buf)
    b.run("nhwc_to_pnc", ("x", xin.off), ("out", out.off), n, p, c, ld)
    got = dev(b, "out")
    tag = f"n{n} p{p} c{c} ld{ld} lead{lead}"
    out.check(got, "nhwc_to_pnc out " + tag)
    assert_same_bits("nhwc_to_pnc data " + tag, out.window(got)[:, :c], want)
    assert not bits(out.window(got)[:, c:]).any(), "nhwc_to_pnc pad columns are not +0: " + tag
    src = Win(p * n, c, ld, 0, data=want, lead=lead)  # pad columns: sentinels
    back = Win(1, n * p * c, lead=lead)
    b.arr("src", src.buf), b.arr("back", back.buf), b.arr("trip", back.buf)
    b.run("pnc_to_nhwc", ("src", src.off), ld, ("back", back.off), n, p, c)
    b.run("pnc_to_nhwc", ("out", out.off), ld, ("trip", back.off), n, p, c)
    for name in ("back", "trip"):
        got = dev(b, name)
        back.check(got, f"pnc_to_nhwc {name} " + tag)
        assert_same_bits(f"pnc_to_nhwc {name} " + tag, back.window(got), x.reshape(1, -1))


def run_layout_c(b, c):
    k = 0
    for ld in ([193] if c == 190 else layout_lds(c)):
        for n, p in LAYOUT_NP:
            run_layout(b, n, p, c, ld, lead=k % 2)  # the base alternates between 16-byte and 4-byte alignment
            k += 1


# ========================================================================================================== 2. LRN
LRN_C = [1, 5, 11, 12, 384]
LRN_RADIUS = [0, 5, "c"]  # "c": a window wider than the row; 5 at c = 11: clipped on one side only at the centre
LRN_ROWS = [1, 3, 257]
LRN_PARAMS = [(1.0, 1.0, 0.5), (2.0, 1e-4, 0.75)]  # (bias, alpha, beta): the shipped set, and one with another beta
LRN_BIG = (43700, 12, 5)  # rows * c = 524 400 > 2048 * 256: the grid stride of both kernels
LRN_REGIMES = ["unit", "1e3", "1e-3", "zero", "1e15"]


def lrn_rows(rows, c, first, rng):
    """row i is of regime (first + i) % 5: unit normal; scale 1e3 (s is the sum); scale 1e-3 (s is about the bias); all
    zero; unit normal with one element of magnitude 1e15 (its square, 1e30, is finite in fp32)"""
    x = rng.standard_normal((rows, c))
    reg = (first + np.arange(rows)) % len(LRN_REGIMES)
    x[reg == 1] *= 1e3
    x[reg == 2] *= 1e-3
    x[reg == 3] = 0.0
    big = np.flatnonzero(reg == 4)
    x[big, big % c] = 1e15 * np.where(big % 2, -1.0, 1.0)
    return x.astype(F32), reg


def window_sum(t, radius):
    """out[:, j] = sum over |k - j| <= radius, k inside the row, of t[:, k]: the terms of that window only, added one
    by one in the dtype of t"""
    rows, c = t.shape
    r = min(int(radius), c - 1)
    tp = np.zeros((rows, c + 2 * r), t.dtype)
    tp[:, r:r + c] = t
    out = np.zeros_like(t)
    for d in range(2 * r + 1):
        out = out + tp[:, d:d + c]
    return out


def lrn_eval(x, g, radius, bias, alpha, beta, dtype):
    """tf.nn.local_response_normalization and its gradient from the definition, in `dtype` (float64: the reference;
    float32: the yardstick):  s_j = bias + alpha * sum_{|k-j|<=r} x_k^2,  y_j = x_j s_j^-beta,
    dx_j = g_j s_j^-beta - 2 alpha beta x_j sum_{|k-j|<=r} g_k x_k s_k^(-beta-1).  Also the two magnitudes of dx."""
    x, g = x.astype(dtype), g.astype(dtype)
    bias, alpha, beta = dtype(bias), dtype(alpha), dtype(beta)
    s = bias + alpha * window_sum(x * x, radius)
    p0, p1 = np.power(s, -beta), np.power(s, -beta - dtype(1))
    y = x * p0
    dx = g * p0 - dtype(2) * alpha * beta * x * window_sum(g * x * p1, radius)
    return y, dx, s, p1


def lrn_bounds(x, g, radius, bias, alpha, beta, powf_ulp):
    """Roundings, in units of U.  w_j = length of the (clipped) window of column j, W = the longest window of the row,
    P0 / P1 = error of the device powf(s, -beta) / powf(s, -beta - 1) in ulps (measured, times the margin; an ulp is at
    most 2 U of the value, and never less than the subnormal spacing 2^-149).

    s_j: each x_k^2 one rounding, the chain of w_j additions w_j - 1 (the first, to 0, is exact), alpha * and bias +
      one each; every term is non-negative, so these relative errors do not grow: (w_j + 2) U of s_j.
    forward: powf turns a relative error e of s into beta * e, adds its own 2 P0 U, and the product with x_j rounds once:
      |y - y64| <= (beta (w_j + 2) + 2 P0 + 1) U |y|.      No cancellation anywhere.
    backward, first term g_j powf(s_j, -beta): (beta (w_j + 2) + 2 P0 + 1) U |g_j| s_j^-beta.
      second term: powf(s_k, -beta - 1) carries (beta + 1)(w_k + 2) U + 2 P1 U (+ P1 2^-149 absolute: at s = 1e30 the
      value is a subnormal); g_k x_k rounds once, its product with the power once, the chain of the window sum w_j - 1
      times; the coefficient ((2 alpha) beta) x_j times the sum rounds 3 times (2 alpha is exact):
      ((beta + 1)(W + 2) + 2 P1 + w_j + 4) U of 2 alpha beta |x_j| sum_k |g_k x_k| s_k^(-beta-1).
      The subtraction rounds once, relative to at most the sum of the two magnitudes: + 1 in both coefficients.
    The two terms cancel (dx is small where the window's own gradient opposes g_j), so the bound is relative to the sum
    of the magnitudes, not to dx.  Absolute floors: each power's P1 2^-149 and each product's TINY, times the
    coefficient; 2 TINY for the last two roundings.
    accumulate (added by the caller): one more rounding, U (|old| + |dx64| + the bound above)."""
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    y, dx, s, p1 = lrn_eval(x, g, radius, bias, alpha, beta, np.float64)
    b64, a64 = float(F32(beta)), float(F32(alpha))
    w = window_sum(np.ones_like(x64), radius)
    W = w.max()
    P0, P1 = powf_ulp[(b64, "fwd")], powf_ulp[(b64, "bwd")]
    fwd = ((b64 * (w + 2) + 2 * P0 + 1) * U * np.abs(y) + TINY) * SLACK
    m1 = np.abs(g64) * np.power(s, -b64)
    coef = 2 * a64 * b64 * np.abs(x64)
    m2 = coef * window_sum(np.abs(g64 * x64) * p1, radius)
    floor = coef * window_sum(np.abs(g64 * x64) * P1 * 2.0 ** -149 + TINY, radius) + 2 * TINY
    bwd = ((b64 * (w + 2) + 2 * P0 + 2) * U * m1 + ((b64 + 1) * (W + 2) + 2 * P1 + w + 5) * U * m2 + floor) * SLACK
    return y, dx, fwd, bwd


def run_lrn(b, rep, rows, c, radius, params, first, powf_ulp):
    """One (rows, c, radius, parameter set): forward, backward and accumulating backward, every operand with its own
    leading dimension; the rows cycle through LRN_REGIMES from `first`.  An all-zero row gives y = 0 exactly, and its
    dx = dy * bias^-beta is held by the same bound (the second magnitude is 0 there)."""
    bias, alpha, beta = (float(F32(v)) for v in params)
    r = c if radius == "c" else radius
    rng = np.random.default_rng(7 * rows + 13 * c + r + first)
    x, reg = lrn_rows(rows, c, first, rng)
    g = rng.standard_normal((rows, c)).astype(F32)
    old = (rng.standard_normal((rows, c)) * 0.5).astype(F32)
    y64, dx64, fwd, bwd = lrn_bounds(x, g, r, bias, alpha, beta, powf_ulp)
    yf, dxf, _, _ = lrn_eval(x, g, r, bias, alpha, beta, F32)
    lay = ["odd", "aligned"] if first % 2 else ["aligned", "odd"]
    X, G, Y = win(rows, c, lay[0], x), Win(rows, c, c + 2, 2, g), win(rows, c, lay[1])
    D0, D1 = Win(rows, c, c + 5, 3), win(rows, c, lay[0], old)
    for name, a in (("x", X), ("g", G), ("y", Y), ("dx", D0), ("dxa", D1)):
        b.arr(name, a.buf)
    tag = f"rows{rows} c{c} r{r} beta{beta} from {LRN_REGIMES[first % 5]}"
    b.run("lrn_fwd", ("x", X.off), X.ld, rows, c, r, bias, alpha, beta, ("y", Y.off), Y.ld)
    b.run("lrn_bwd", ("x", X.off), X.ld, ("g", G.off), G.ld, rows, c, r, bias, alpha, beta, ("dx", D0.off), D0.ld, 0)
    b.run("lrn_bwd", ("x", X.off), X.ld, ("g", G.off), G.ld, rows, c, r, bias, alpha, beta, ("dxa", D1.off), D1.ld, 1)
    got = dev(b, "y")
    Y.check(got, "lrn_fwd y " + tag)
    hold(rep, f"lrn_fwd beta={beta}", Y.window(got), y64, fwd, yf, tag)
    assert not Y.window(got)[reg == 3].any(), "lrn_fwd: an all-zero row is not exactly 0: " + tag
    got = dev(b, "dx")
    D0.check(got, "lrn_bwd dx " + tag)
    hold(rep, f"lrn_bwd beta={beta}", D0.window(got), dx64, bwd, dxf, tag)
    got = dev(b, "dxa")
    D1.check(got, "lrn_bwd accumulate dx " + tag)
    acc = bwd + U * (np.abs(old.astype(np.float64)) + np.abs(dx64) + bwd) * SLACK
    hold(rep, f"lrn_bwd accumulate beta={beta}", D1.window(got), old.astype(np.float64) + dx64, acc, old + dxf, tag)


def run_lrn_c(b, rep, c, powf_ulp):
    k = 0
    for radius in LRN_RADIUS:
        for rows in LRN_ROWS:
            for params in LRN_PARAMS:
                for first in (range(k, k + 5) if rows == 1 else [k]):  # a single row: once in every regime
                    run_lrn(b, rep, rows, c, radius, params, first, powf_ulp)
                k += 1


# ============================================================================================ 3. MSE, partials, sum
MSE_SHAPES = [(1, 1), (1, 3), (2, 2), (3, 85), (16, 16), (1, 257), (3, 86), (65537, 4)]  # rows * c of {1, 3, 4, 255, 256,
# 257, 1024 * 256 + 4} and 258 (% 4 == 2); 65537 x 4: a thread of either kernel takes a second trip
MSE_FLAT_BIG = (131073, 8)  # 4 * (1024 * 256) + 8: a thread of the flat4 kernel takes a second trip
# how one operand set is presented: (name, layout of a, of b, of da or None)
MSE_FORMS = [("flat", "tight", "tight", "tight"), ("a+1", "tight+1", "tight", "tight"), ("b+1", "tight", "tight+1", "tight"),
             ("da+1", "tight", "tight", "tight+1"), ("lda", "wide", "tight", "tight"), ("ldb", "tight", "wide", "tight"),
             ("ldda", "tight", "tight", "wide"), ("no da", "tight", "tight", None), ("odd", "odd", "odd", "odd")]
GSCALE = float(F32(0.37))


def mse_win(rows, c, layout, data=None):
    return Win(rows, c, c + 4, 0, data) if layout == "wide" else win(rows, c, layout, data)  # wide: aligned, only ld > c


def mse_chain(total, grid):
    """additions a thread makes: the general kernel's chain ceil(total / (grid * 256)), or the flat4 kernel's
    3 per trip ((dx^2 + dy^2) + (dz^2 + dw^2), then + s) over ceil(total / 4 / (grid * 256)) trips -- whichever is more,
    the dispatch being the library's own business"""
    per = grid * 256
    return max(-(-total // per), 3 * -(-(-(-total // 4)) // per))


def mse_bounds(a, b, grid):
    """d = a - b rounds once (U |d|), d * d once more: 3 U of d^2.  Every term is non-negative, so what follows is
    relative to the sum: the per-thread chain (`mse_chain`), the 6 shuffle levels and the 3 additions of block_sum_256,
    and -- hypel_mse only, but allowed to both -- the float64 finaliser's one rounding to fp32: (3 + chain + 6 + 3 + 1) U
    of the sum, plus TINY per term (a d^2 below 1e-38 rounds to a subnormal or to 0).
    da = gcoef * d with gcoef = fl(2 gscale / fl(total)): 2 gscale and total < 2^24 are exact, the division rounds once,
    d once, the product once: 3 U |da| + TINY."""
    total = a.size
    assert total < 2 ** 24
    d = a.astype(np.float64) - b.astype(np.float64)
    sse = float((d * d).sum())
    rel = (3 + mse_chain(total, grid) + 6 + 3 + 1) * U
    da = GSCALE * 2.0 * d / total
    return sse, (rel * sse + total * TINY) * SLACK, da, (3 * U * np.abs(da) + TINY) * SLACK


def mse_yard(a, b):
    d = a - b
    total = F32(a.size)
    return float(np.sum(d * d, dtype=F32)), (F32(GSCALE) * F32(2) / total) * d


def mse_operands(rows, c, kind, rng):
    total = rows * c
    if kind == "one":  # a == b in every element but one: the MSE is that one term
        a = rng.standard_normal((rows, c)).astype(F32)
        b = a.copy()
        b.reshape(-1)[total // 2] += F32(0.75)
    elif kind == "span":  # |a - b| from 1e-20 to 1e15
        d = 10.0 ** rng.uniform(-20, 15, (rows, c)) * rng.choice([-1.0, 1.0], (rows, c))
        a, b = (1.5 * d).astype(F32), (0.5 * d).astype(F32)
    else:
        a, b = rng.standard_normal((rows, c)).astype(F32), rng.standard_normal((rows, c)).astype(F32)
    return a, b


def run_mse(b, rep, rows, c, kind="normal", forms=MSE_FORMS):
    """hypel_mse and hypel_mse_partial_f32 on one operand set in every form of MSE_FORMS, each result against the same
    float64 reference.  Outside the windows of da, `out` and the 1024 floats of ws nothing is written; with da == NULL
    a and b keep their bits too.  hypel_mse_partial_f32: ws holds sentinels over 1024 + 8 floats; afterwards exactly the
    first 1024 are written, each finite and >= 0, their float64 sum within the bound -- and with rows * c = 3 every
    partial but one is +0 (a block without elements publishes +0)."""
    rng = np.random.default_rng(31 * rows + c + len(kind))
    a, bb = mse_operands(rows, c, kind, rng)
    total = rows * c
    ysse, yda = mse_yard(a, bb)
    for form, la, lb, lda in forms:
        A, B = mse_win(rows, c, la, a), mse_win(rows, c, lb, bb)
        D = None if lda is None else mse_win(rows, c, lda)
        tag = f"{rows}x{c} {kind} {form}"
        for entry in ("mse", "mse_partial_f32"):
            grid = MSE_PARTIALS if entry == "mse_partial_f32" else min(-(-total // 256), RED_BLOCKS)
            sse, sse_bound, da64, da_bound = mse_bounds(a, bb, grid)
            WS, OUT = Win(1, MSE_PARTIALS + (8 if entry == "mse_partial_f32" else 0), lead=1), Win(1, 1, lead=3)
            b.arr("a", A.buf), b.arr("b", B.buf), b.arr("ws", WS.buf), b.arr("out", OUT.buf)
            dref, ldd = None, 0
            if D is not None:
                b.arr("da", D.buf)
                dref, ldd = ("da", D.off), D.ld
            if entry == "mse":
                b.run("mse", ("a", A.off), A.ld, ("b", B.off), B.ld, rows, c, ("out", OUT.off), dref, ldd, GSCALE, ("ws", WS.off))
                got = dev(b, "out")
                OUT.check(got, "mse out " + tag)
                hold(rep, "mse", OUT.window(got), sse / total, sse_bound / total, ysse / total, tag)
                WS.check(dev(b, "ws"), "mse ws " + tag)
            else:
                b.run("mse_partial_f32", ("a", A.off), A.ld, ("b", B.off), B.ld, rows, c, dref, ldd, GSCALE, ("ws", WS.off))
                got = dev(b, "ws")
                WS.check(got, "mse_partial ws " + tag)
                part = WS.window(got)[0]
                assert (bits(part[MSE_PARTIALS:]) == bits(SENT)).all(), "more than 1024 partials written: " + tag
                head = part[:MSE_PARTIALS]
                assert (bits(head) != bits(SENT)).all() and np.isfinite(head).all() and (head >= 0).all(), tag
                if total == 3:
                    assert np.count_nonzero(bits(head)) <= 1, "a block without elements did not publish +0: " + tag
                hold(rep, "mse_partial sum", head.astype(np.float64).sum(), sse, sse_bound, ysse, tag)
                assert_same_bits("out untouched " + tag, dev(b, "out"), OUT.buf)
            if D is not None:
                got = dev(b, "da")
                D.check(got, f"{entry} da " + tag)
                hold(rep, "mse da", D.window(got), da64, da_bound, yda, tag)
            else:
                assert_same_bits("a " + tag, dev(b, "a"), A.buf), assert_same_bits("b " + tag, dev(b, "b"), B.buf)


SUM_COUNTS = [1, 3, 4, 255, 256, 257, 1024 * 256 + 4]
SUM_SCALE = float(F32(0.37))


def sum_grid(count):
    return min(-(-count // 256), RED_BLOCKS)


def run_sum(b, rep, x, label, exact_zero=False):
    """hypel_sum_f32 = sum(x) * scale: a thread's chain of ceil(count / (grid * 256)) additions, 6 shuffle levels and 3
    additions in the block, a float64 finaliser and its rounding to fp32: (chain + 6 + 3 + 1) U of sum |x| * scale.  x once
    at a 16-byte base and once one float behind it."""
    count = x.size
    ref = float(np.sum(x.astype(np.float64))) * SUM_SCALE
    mag = float(np.abs(x.astype(np.float64)).sum()) * SUM_SCALE
    bound = ((-(-count // (sum_grid(count) * 256)) + 10) * U * mag + TINY) * SLACK
    yard = float(np.sum(x, dtype=F32) * F32(SUM_SCALE))
    for lead in (0, 1):
        X, WS, OUT = Win(1, count, data=x, lead=lead), Win(1, MSE_PARTIALS, lead=1), Win(1, 1, lead=3)
        b.arr("x", X.buf), b.arr("ws", WS.buf), b.arr("out", OUT.buf)
        b.run("sum_f32", ("x", X.off), count, SUM_SCALE, ("out", OUT.off), ("ws", WS.off))
        got = dev(b, "out")
        OUT.check(got, f"sum_f32 out {label}"), WS.check(dev(b, "ws"), f"sum_f32 ws {label}")
        if exact_zero:
            assert OUT.window(got)[0, 0] == 0.0, f"sum_f32 {label}: pairs inside one chain must cancel exactly"
        hold(rep, "sum_f32", OUT.window(got), ref, bound, yard, f"{label} lead {lead}")


def sum_pairs_in_chain(rng):
    """2 * G elements with G = grid * 256 threads: thread t adds x[t], then x[t + G] = -x[t]: every chain is exactly +0"""
    G = RED_BLOCKS * 256
    v = (rng.standard_normal(G) * 10.0 ** rng.uniform(-3, 3, G)).astype(F32)
    x = np.concatenate([v, -v])
    assert sum_grid(x.size) * 256 == G and (x[:G] == -x[G:]).all() and x.size == 2 * G  # from the indices
    return x


def sum_pairs_across_blocks(rng):
    """1024 elements, one per thread of 4 blocks: +v in blocks 0 and 1, -v in blocks 2 and 3"""
    v = (rng.standard_normal(512) * 10.0 ** rng.uniform(-3, 3, 512)).astype(F32)
    x = np.concatenate([v, -v])
    assert sum_grid(x.size) == 4
    return x


# =========================================================================================================== 4. argmax
ARGMAX_C = [1, 2, 15, 20, 256]
ARGMAX_N = [1, 127, 128, 129]
ROW_KINDS = ["max at 0", "max in the middle", "max at c-1", "2-way tie", "3-way tie", "all equal", "all -inf", "-0 then +0",
             "+0 then -0", "one ulp", "+inf", "NaN at 0", "NaN in the middle", "NaN at c-1", "all NaN"]


def argmax_rows(n, c, first, rng):
    """row i is of kind (first + i) % 15 (ROW_KINDS); -> (logits [n, c], kind per row)"""
    z = rng.standard_normal((n, c)).astype(F32)
    kind = (first + np.arange(n)) % len(ROW_KINDS)
    mid = c // 2
    for i in range(n):
        k, r = kind[i], z[i]
        cols = sorted({(i * 5) % c, (i * 5 + 1 + i % 3) % c, (i * 7 + 2) % c})  # up to three distinct columns, ascending
        if k == 0:
            r[0] = 9.0
        elif k == 1:
            r[mid] = 9.0
        elif k == 2:
            r[c - 1] = 9.0
        elif k == 3:
            r[cols[:2]] = 7.0
        elif k == 4:
            r[cols] = 7.0
        elif k == 5:
            r[:] = 0.25
        elif k == 6:
            r[:] = -np.inf
        elif k in (7, 8):  # +0 against -0 is a tie: the first wins
            r[:] = -1.0
            r[cols[0]] = -0.0 if k == 7 else 0.0
            r[cols[-1]] = 0.0 if k == 7 else -0.0
        elif k == 9:
            r[:] = 3.0
            r[cols[-1]] = np.nextafter(F32(3.0), F32(4.0))
        elif k == 10:
            r[cols[0]] = r[cols[-1]] = np.inf
        elif k == 11:
            r[0] = np.nan
        elif k == 12:
            r[mid] = np.nan
            r[cols[0]] = 8.0 if cols[0] != mid else np.nan
        elif k == 13:
            r[c - 1] = np.nan
        elif k == 14:
            r[:] = np.nan
    return z, kind


def first_max(z):
    """include/hypel.h: one pass from column 0 that moves on `>`; rows without NaN: numpy.argmax"""
    best, bv = np.zeros(len(z), np.int64), z[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for j in range(1, z.shape[1]):
            m = z[:, j] > bv
            bv[m], best[m] = z[m, j], j
    clean = ~np.isnan(z).any(1)
    assert (best[clean] == np.argmax(z[clean], 1)).all()
    return best


def logits_buffer(z, ld, lead):
    """[n x c] at column 0 of rows of ld floats whose pad holds +inf: a kernel that reads the pad picks it"""
    n, c = z.shape
    buf = np.full(lead + n * ld + 5, np.inf, F32)
    buf[lead:lead + n * ld].reshape(n, ld)[:, :c] = z
    return buf


def argmax_labels(n, c, rng):
    lab = rng.integers(0, c, n).astype(np.int32)
    lab[2::5] = np.resize(np.asarray([-1, c, 255], np.int32), len(lab[2::5]))  # outside [0, c) (255 is a class at c = 256)
    return lab


def confusion_of(lab, pred, c):
    known = (lab >= 0) & (lab < c)
    return np.bincount(lab[known].astype(np.int64) * c + pred[known], minlength=c * c).astype(np.int32)


def run_argmax_confusion(b, n, c, ld, first):
    """Predictions bit exact against `first_max` (numpy.argmax on every row without a NaN); labels outside [0, c) are not
    counted; a second launch into the same table accumulates; pred, confusion, labels each NULL on its own leave the
    other outputs as specified and everything else untouched."""
    rng = np.random.default_rng(100 * c + n + ld)
    z, _ = argmax_rows(n, c, first, rng)
    lead = first % 2 * 3
    lab = argmax_labels(n, c, rng)
    pred = first_max(z)
    counts = confusion_of(lab, pred, c)
    conf0 = rng.integers(0, 50, c * c).astype(np.int32)
    tag = f"n{n} c{c} ld{ld}"
    b.arr("z", logits_buffer(z, ld, lead)), b.arr("lab", lab)
    for mode, fresh in (("all", True), ("all", False), ("no pred", True), ("no confusion", True), ("no labels", True)):
        if fresh:
            P, C = IntGuard(n), IntGuard(c * c, init=conf0)
            b.arr("pred", P.buf), b.arr("conf", C.buf)
            launches = 0
        b.run("argmax_confusion", ("z", lead), ld, n, c, None if mode == "no labels" else "lab",
              None if mode == "no pred" else ("pred", P.off), None if mode == "no confusion" else ("conf", C.off))
        launches += 1
        gp, gc = dev(b, "pred"), dev(b, "conf")
        P.check(gp, "pred " + tag), C.check(gc, "confusion " + tag)
        want_p = np.full(n, ISENT) if mode == "no pred" else pred
        want_c = conf0 + (launches * counts if mode in ("all", "no pred") else 0)
        assert (P.payload(gp) == want_p).all(), f"pred ({mode}) {tag}: rows {np.flatnonzero(P.payload(gp) != want_p)[:8]}"
        assert (C.payload(gc) == want_c).all(), f"confusion ({mode}, launch {launches}) {tag}"
    assert_same_bits("logits " + tag, dev(b, "z"), logits_buffer(z, ld, lead))


def run_confusion_one_cell(b, n=129, c=15):
    """all n rows predict class 11 with label 4: n atomics on one address"""
    z = np.zeros((n, c), F32)
    z[:, 11] = 1.0
    C = IntGuard(c * c, init=np.zeros(c * c, np.int32))
    b.arr("z", z), b.arr("lab", np.full(n, 4, np.int32)), b.arr("conf", C.buf)
    b.run("argmax_confusion", "z", c, n, c, "lab", None, ("conf", C.off))
    got = dev(b, "conf")
    C.check(got, "confusion")
    want = np.zeros(c * c, np.int32)
    want[4 * c + 11] = n
    assert (C.payload(got) == want).all()


def scatter_points(n, h, w, rng):
    """n distinct (x, y), the four raster corners first"""
    corners = list(dict.fromkeys([(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]))
    rest = [(x, y) for y in range(h) for x in range(w) if (x, y) not in corners]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    pts = (corners + rest)[:n]
    assert len(pts) == n
    return np.asarray(pts, np.int32)


def run_argmax_scatter(b, n, c, ld, first, raster_w):
    """raster[y * raster_w + x] = first_max(logits[i]) as a byte (c = 256 writes 255); every byte not addressed keeps
    its fill, in the raster and round it"""
    rng = np.random.default_rng(200 * c + n + ld + raster_w)
    z, _ = argmax_rows(n, c, first, rng)
    h = n + 2 if raster_w == 1 else -(-(n + 9) // raster_w)
    pts = scatter_points(n, h, raster_w, rng)
    fill = np.uint8(200)
    R = IntGuard(h * raster_w, np.uint8, init=fill, g=61)
    lead = first % 2
    b.arr("z", logits_buffer(z, ld, lead)), b.arr("pts", pts), b.arr("raster", R.buf)
    b.run("argmax_scatter", ("z", lead), ld, n, c, "pts", ("raster", R.off), raster_w)
    got = dev(b, "raster")
    R.check(got, "raster")
    want = np.full((h, raster_w), fill)
    want[pts[:, 1], pts[:, 0]] = first_max(z).astype(np.uint8)
    assert (R.payload(got).reshape(h, raster_w) == want).all(), f"argmax_scatter n{n} c{c} ld{ld} w{raster_w}"
    return want


def run_argmax_c(b, c):
    k = 0
    for n in ARGMAX_N:
        for ld in (c, c + 3):
            run_argmax_confusion(b, n, c, ld, k)
            for raster_w in (13, 1):
                want = run_argmax_scatter(b, n, c, ld, k, raster_w)
                k += 1
    if c == 256:
        assert (want == 255).any()  # n = 129 holds rows whose maximum is the last column


# ========================================================================================== 5. gathers, augmentation
GATHER_CC_CL = [(t - cl, cl) for t in (95, 96, 191, 192, 193) for cl in (0, 1, 3)]  # the 64 / 128 / 256-lane block choice
GATHER_BIG = (911, 3)  # n * p * p = 8199 > 8192: a block walks to a second item


def gather_scene(hp, wp, cc, cl, rng):
    casi = rng.standard_normal((hp, wp, cc)).astype(F32)
    lidar = rng.standard_normal((hp, wp, max(cl, 1))).astype(F32)[:, :, :cl]
    return casi, lidar


def run_gather(b, cc, cl, p, n, hp=6, wp=7):
    """out[i] = concat(casi[y:y+p, x:x+p], lidar[y:y+p, x:x+p]) for point i = (x, y): NumPy slicing.  The points start
    with the four corners of the valid area, whose patches touch the first and last padded row and column."""
    rng = np.random.default_rng(cc * 10 + cl + p + n)
    casi, lidar = gather_scene(hp, wp, cc, cl, rng)
    corners = [(wp - p, hp - p), (0, 0), (wp - p, 0), (0, hp - p)]
    pts = np.asarray((corners + [(int(rng.integers(0, wp - p + 1)), int(rng.integers(0, hp - p + 1))) for _ in range(n)])[:n],
                     np.int32)
    want = np.stack([np.concatenate([casi[y:y + p, x:x + p], lidar[y:y + p, x:x + p]], -1) for x, y in pts])
    CA, LI = Win(1, casi.size, data=casi, lead=1), Win(1, max(lidar.size, 1), data=lidar if cl else None, lead=2)
    for lead in (0, 1):
        O = Win(1, want.size, lead=lead)
        b.arr("casi", CA.buf), b.arr("lidar", LI.buf), b.arr("pts", pts), b.arr("out", O.buf)
        b.run("gather_patches_f32", ("casi", CA.off), ("lidar", LI.off) if cl else None, hp, wp, cc, cl, "pts", n, p,
              ("out", O.off))
        got = dev(b, "out")
        tag = f"gather cc{cc} cl{cl} p{p} n{n} lead{lead}"
        O.check(got, tag)
        assert_same_bits(tag, O.window(got), want.reshape(1, -1))


def loader_patch_2x(casi, lidar, nb, x, y):
    """GRSS2018DataSet.get_data_point: the spectrum of the half-resolution pixel under each LiDAR pixel, the heights of
    the LiDAR window; both rasters padded by nb; start = int(coordinate * scale) + nb - int(nb * scale)"""
    size = 2 * nb + 1
    sx, sy = int(x * 0.5) + nb - int(nb * 0.5), int(y * 0.5) + nb - int(nb * 0.5)
    half = (np.arange(size) * 0.5).astype(int)
    return np.concatenate([casi[sy + half[:, None], sx + half[None, :], :], lidar[y:y + size, x:x + size, :]], -1)


def run_gather_2x(b, nb, cc, cl, n=None, h=6, w=7):
    """every (x, y) of a 6 x 7 LiDAR grid -- all four parities, the corners of the valid area -- at nb in {0, 1, 2, 3}
    (both parities of nb), p = 2 nb + 1, against `loader_patch_2x`"""
    rng = np.random.default_rng(nb * 100 + cc)
    p = 2 * nb + 1
    casi = rng.standard_normal(((h + 1) // 2 + 2 * nb, (w + 1) // 2 + 2 * nb, cc)).astype(F32)
    lidar = rng.standard_normal((h + 2 * nb, w + 2 * nb, cl)).astype(F32)
    pts = np.asarray([(x, y) for y in range(h) for x in range(w)], np.int32)[::-1][:n]
    want = np.stack([loader_patch_2x(casi, lidar, nb, int(x), int(y)) for x, y in pts])
    CA, LI = Win(1, casi.size, data=casi, lead=1), Win(1, lidar.size, data=lidar, lead=2)
    O = Win(1, want.size, lead=nb % 2)
    b.arr("casi", CA.buf), b.arr("lidar", LI.buf), b.arr("pts", pts), b.arr("out", O.buf)
    b.run("gather_patches_2x_f32", ("casi", CA.off), ("lidar", LI.off), casi.shape[1], lidar.shape[1], cc, cl, nb, "pts",
          len(pts), p, ("out", O.off))
    got = dev(b, "out")
    tag = f"gather_2x nb{nb} cc{cc} cl{cl} n{len(pts)}"
    O.check(got, tag)
    assert_same_bits(tag, O.window(got), want.reshape(1, -1))


AUGMENT_C = [95, 96, 192]
AUGMENT_SELECTORS = [(), ("rot_k",), ("ratio",), ("alt",), ("flip_lr",), ("flip_ud",), ("delta",),
                     ("rot_k", "ratio", "flip_lr", "flip_ud", "delta"), ("rot_k", "alt", "flip_lr", "flip_ud", "delta")]


def run_augment(b, c, n, p, selectors, with_idx):
    """against the torch / NumPy composition of tests/test_data_side.py (rot90 -> shadow -> flips -> shift), bit exact;
    rot_k holds 3; idx NULL is the identity gather"""
    from tests.test_data_side import torch_augment
    rng = np.random.default_rng(c + 10 * n + p + len(selectors))
    pool = rng.random((n + (3 if with_idx else 0), p, p, c), dtype=np.float32) + F32(0.5)
    idx = rng.integers(0, len(pool), n).astype(np.int64) if with_idx else None
    d, ratio, alt = {}, None, None
    if "rot_k" in selectors:
        d["rot_k"] = torch.tensor(np.resize(np.asarray([3, 1, 2, 0, 3, 1], np.int32), n))
    if "ratio" in selectors or "alt" in selectors:
        d["shadow_pick"] = torch.tensor(np.resize(np.asarray([1, 0, 1, 1, 0, 1], np.uint8), n))
        if "ratio" in selectors:
            ratio = rng.uniform(1.2, 3.0, c).astype(F32)
        else:
            alt = rng.random((n, p, p, c), dtype=np.float32)
    for k in ("flip_lr", "flip_ud"):
        if k in selectors:
            d[k] = torch.tensor(np.resize(np.asarray([1, 1, 0, 1, 0, 0] if k == "flip_lr" else [1, 0, 1, 1, 0, 1], np.uint8), n))
    if "delta" in selectors:
        d["delta"] = torch.tensor((rng.random((n, c)) * 0.05 - 0.05).astype(F32))
    src = torch.tensor(pool if idx is None else pool[idx])
    want = torch_augment(src, d, None if ratio is None else torch.tensor(ratio), None if alt is None else torch.tensor(alt)).numpy()
    O = Win(1, want.size, lead=len(selectors) % 2)
    b.arr("x", pool), b.arr("out", O.buf)
    names = {}
    for k, v in (("idx", idx), ("ratio", ratio), ("alt", alt)) + tuple((k, v.numpy()) for k, v in d.items()):
        names[k] = None if v is None else b.arr(k, v)
    b.run("augment_patches_f32", "x", names["idx"], n, p, c, names.get("rot_k"), names.get("shadow_pick"), names["ratio"],
          names["alt"], names.get("flip_lr"), names.get("flip_ud"), names.get("delta"), ("out", O.off))
    got = dev(b, "out")
    tag = f"augment c{c} n{n} p{p} {'+'.join(selectors) or 'plain'} idx={with_idx}"
    O.check(got, tag)
    assert_same_bits(tag, O.window(got), want.reshape(1, -1))


def run_augment_c(b, c):
    for k, sel in enumerate(AUGMENT_SELECTORS):
        for n in (1, 6):
            run_augment(b, c, n, 3 if k % 2 else 2, sel, with_idx=(k + n) % 2 == 0)
            run_augment(b, c, n, 3 if k % 2 else 2, sel, with_idx=(k + n) % 2 == 1)


def run_augment_refusal(backend):
    """shadow_ratio and shadow_alt together: refused before any launch (the emulation asserts), `out` untouched.
    -> the message"""
    from hypelcnn_amd.backend import Ref
    n, p, c = 2, 2, 5
    O = Win(1, n * p * p * c, lead=1)
    up = lambda a: Ref(backend.upload(a))  # noqa: E731
    out = backend.upload(O.buf)
    with pytest.raises((HypelError, AssertionError)) as e:
        backend.call("augment_patches_f32", up(np.ones(n * p * p * c, F32)), None, n, p, c, None, up(np.ones(n, np.uint8)),
                     up(np.full(c, 2.0, F32)), up(np.zeros(n * p * p * c, F32)), None, None, None, Ref(out, O.off))
    backend.synchronize()
    assert_same_bits("out after the refused call", out.cpu().numpy(), O.buf)
    return str(e.value)


# ====================================================================================== 6. chanmap_bwd, copies
CHANMAP_TABLES = {1: (7, [0, 7]), 3: (9, [0, 0, 9, 9]), 4: (10, [0, 3, 3, 4, 10])}  # cin -> (c, start): empty ranges, all of c
CHANMAP_CIN = [1, 3, 4, 60]
CHANMAP_ROWS = [1, 257]


def chanmap_table(cin):
    if cin in CHANMAP_TABLES:
        return CHANMAP_TABLES[cin]
    lens = [2] * cin  # cin = 60 over c = 145: ranges of 2, two empty ones in a row and a third, lengths 1 and 3, one of 33
    lens[7] = lens[8] = lens[20] = 0
    lens[40], lens[41] = 1, 3
    lens[33] += 145 - sum(lens)
    return 145, [0] + [int(v) for v in np.cumsum(lens)]


def run_chanmap(b, rep, cin, rows, layout, accumulate, table):
    """dr[row][k] (+)= sum of dz[row][start[k] : start[k + 1]].  With a table: float64 reference; a range of L terms is
    a chain of L - 1 roundings (the first addition, to 0, is exact), relative to the sum of magnitudes: L U sum |dz|;
    an empty range gives exactly 0; accumulate adds one rounding, U (|old| + |sum| + the bound so far).  Without a
    table (cin == c): a copy, or one fp32 addition -- bit exact against np.float32 arithmetic."""
    c, start = chanmap_table(cin) if table else (cin, None)
    rng = np.random.default_rng(cin * 1000 + rows + accumulate)
    dz = rng.standard_normal((rows, c)).astype(F32)
    old = rng.standard_normal((rows, cin)).astype(F32)
    DZ, DR = win(rows, c, "odd" if table else layout, dz), win(rows, cin, layout, old if accumulate else None)
    b.arr("dz", DZ.buf), b.arr("dr", DR.buf)
    if table:
        b.arr("start", np.asarray(start, np.int32))
    b.run("chanmap_bwd", ("dz", DZ.off), DZ.ld, rows, c, ("dr", DR.off), DR.ld, cin, "start" if table else None, accumulate)
    got = dev(b, "dr")
    tag = f"chanmap_bwd cin{cin} rows{rows} {layout} acc{accumulate} table{table}"
    DR.check(got, tag)
    if not table:
        assert_same_bits(tag, DR.window(got), old + dz if accumulate else dz)
        return
    st = np.asarray(start)
    d64 = dz.astype(np.float64)
    ref = np.stack([d64[:, a:e].sum(1) for a, e in zip(st[:-1], st[1:])], 1)
    mag = np.stack([np.abs(d64[:, a:e]).sum(1) for a, e in zip(st[:-1], st[1:])], 1)
    yard = np.stack([np.sum(dz[:, a:e], 1, dtype=F32) for a, e in zip(st[:-1], st[1:])], 1)
    bound = (st[1:] - st[:-1])[None, :] * U * mag * SLACK
    if accumulate:
        bound = bound + U * (np.abs(old) + np.abs(ref) + bound) * SLACK
        ref, yard = ref + old, yard + old
    empty = st[1:] == st[:-1]
    assert_same_bits(tag + " empty ranges", DR.window(got)[:, empty], old[:, empty] if accumulate else np.zeros((rows, empty.sum())))
    hold(rep, "chanmap_bwd", DR.window(got), ref, bound, yard, tag)


def run_copy_blocks(b):
    """Entries for which exactly one of the four float4 conditions fails (cols % 4, src_ld % 4, dst_ld % 4, a 16-byte
    base on either side), and one for which none does, each as a copy and as an accumulate, plus a block of two grid
    rows; the whole buffer bit for bit against NumPy (accumulate: one np.float32 addition)."""
    rng = np.random.default_rng(77)
    forms = [("v4", 8, 12, 16, 0, 0), ("cols", 7, 12, 16, 0, 0), ("src_ld", 8, 13, 16, 0, 0), ("dst_ld", 8, 12, 17, 0, 0),
             ("src base", 8, 12, 16, 1, 0), ("dst base", 8, 12, 16, 0, 2)]
    specs = [(5, cols, sld, dld, so, do, acc) for _, cols, sld, dld, so, do in forms for acc in (0, 1)]
    specs += [(40, 64, 64, 68, 0, 0, 0), (40, 64, 67, 64, 0, 0, 1)]  # 2560 elements: two blocks along y
    ents, chunks, pos = [], [], 64
    for rows, cols, sld, dld, so, do, acc in specs:
        src = pos + so
        pos = roundup4(src + rows * sld) + 32
        dst = pos + do
        pos = roundup4(dst + rows * dld) + 32
        chunks.append((rows, cols, sld, dld, src, dst, acc))
        ents.append((src, dst, rows, cols, sld, dld, acc, 0))
    buf = np.full(pos + 64, SENT, F32)
    for rows, cols, sld, dld, src, dst, acc in chunks:
        si = src + np.arange(rows)[:, None] * sld + np.arange(cols)[None, :]
        di = dst + np.arange(rows)[:, None] * dld + np.arange(cols)[None, :]
        buf[si] = rng.standard_normal((rows, cols)).astype(F32)
        if acc:
            buf[di] = rng.standard_normal((rows, cols)).astype(F32)
    want = buf.copy()
    for rows, cols, sld, dld, src, dst, acc in chunks:
        si = src + np.arange(rows)[:, None] * sld + np.arange(cols)[None, :]
        di = dst + np.arange(rows)[:, None] * dld + np.arange(cols)[None, :]
        want[di] = want[di] + buf[si] if acc else buf[si]
    b.arr("buf", buf), b.arr("ents", np.array(ents, COPY_BLOCK_DTYPE))
    b.run("copy_blocks_f32", "buf", "ents", len(ents), max(e[2] * e[3] for e in ents))
    assert_same_bits("copy_blocks", dev(b, "buf"), want)


COPY_PAIR_COUNTS = [0, 1, 3, 4, 5]


def run_copy_pair(b):
    """counts {0, 1, 3, 4, 5} on either side, the sources at a 16-byte base and one float behind it"""
    rng = np.random.default_rng(5)
    s0, s1 = rng.standard_normal(16).astype(F32), rng.standard_normal(16).astype(F32)
    for off in (0, 1):
        for n0 in COPY_PAIR_COUNTS:
            for n1 in COPY_PAIR_COUNTS:
                D0, D1 = Win(1, max(n0, 1)), Win(1, max(n1, 1))
                b.arr("s0", s0), b.arr("s1", s1), b.arr("d0", D0.buf), b.arr("d1", D1.buf)
                b.run("copy_pair_f32", ("d0", D0.off), ("s0", off), n0, ("d1", D1.off), ("s1", off), n1)
                for name, D, s, n in (("d0", D0, s0, n0), ("d1", D1, s1, n1)):
                    want = D.buf.copy()
                    want[D.off:D.off + n] = s[off:off + n]
                    assert_same_bits(f"copy_pair {name} n0={n0} n1={n1} off={off}", dev(b, name), want)
