"""The batch-norm chain of csrc/elementwise.hip, written down three times (CPU, NumPy only):

1. DEFINITIONS in float64, straight from the mathematics (not through tests/emu_backend.py): column mean, biased
   variance, rstd = 1 / sqrt(var + eps), moving averages with the Bessel-corrected variance (the biased one when
   rows == 1), forward act((y - mean) * rstd + beta) * mask + res, backward dyh = dz * mask * act'(pre),
   s0 = sum dyh, s1 = sum dyh * xhat, dy = rstd * (dyh - s0 / N - xhat * s1 / N), dbeta (+)= s0, and the multi-rank
   merge as the statistics of the concatenated rows.

2. An fp32 TWIN of the statistics path.  It has the kernels' STRUCTURE, not their code: per chunk, d = x - x[first
   row of the chunk] and d * d are added in float32, first down each row lane (rows r0 + lane, r0 + lane + LANES, ..),
   then across the lanes; m2 = sum d^2 - (sum d)^2 / n; the chunk records are merged in float64.  Three NAIVE twins
   (E[x^2] - mean^2 in fp32, an unshifted fp32 sum, an fp32 merge of the chunk records) show what the bounds reject.

3. BOUNDS, as functions of the data, in units of U = 2^-24 (one fp32 rounding moves a value v by at most U |v|).

   One chunk of n rows.  Write d_r = x_r - x_0 (exact), S = sum d, A = sum |d|, D2 = sum d^2, and L for the longest
   chain of additions a term passes through: ceil(n / LANES) down its lane plus CROSS across the lanes (FORMS).
     d-hat = fl(x_r - x_0) = d (1 + e1)                                                          one rounding
     s-hat = sum-hat d-hat = sum d (1 + e1)(1 + theta), |theta| <= L U   ->  |s-hat - S| <= (L + 1) U A
     mean_k = fl(x_0 + fl(s-hat / n)):  the division adds U |S| / n <= U A / n, the addition U |mean_k|
         |mean_k - true| <= (L + C_MEAN) U A / n + U |mean_k|,                                   C_MEAN = 2
     q-hat = sum-hat fl(d-hat^2): (1 + e1)^2 and the product's rounding are 3 U, the additions L U
         |q-hat - D2| <= (L + C_SQ) U D2,                                                         C_SQ = 3
     p-hat = fl(s-hat * fl(s-hat / n)): |s-hat^2 - S^2| / n <= 2 |S| (L + 1) U A / n, two roundings 2 U S^2 / n, and
         S^2 <= |S| A:   |p-hat - S^2 / n| <= 2 (L + C_MEAN) U |S| A / n      (<= 2 (L + C_MEAN) U D2: Cauchy-Schwarz)
     m2_k = fl(q-hat - p-hat) (the clamp at 0 only moves it towards the true value, which is >= 0):
         |m2_k - true| <= (L + C_SQ) U D2 + 2 (L + C_MEAN) U |S| A / n + U |M2_k|
   The squared-sum term is what makes a column whose first chunk row is an outlier (family d) the worst case: there
   |S| A / n is as large as D2 while the true M2 is much smaller.  Fused multiply-adds only remove roundings.

   Merge of K records (n_k, mean_k +- e_k, M2_k +- f_k) in float64 (its own rounding, 2^-53, is inside SLACK):
     mean = sum n_k mean_k / N                 ->  e_mean = sum n_k e_k / N
     M2 = sum M2_k + n_k (mean_k - mean)^2     ->  every deviation moves by at most g_k = e_k + e_mean, so
         e_M2 = sum f_k + sum n_k (2 |mean_k - mean| g_k + g_k^2)                 (exact in g_k, not first order)
   Results stored as float32 take one more rounding U |value|; rstd = 1 / sqrt(var + eps) is monotone in var, so its
   bound is the larger one-sided change over [var - e, var + e] (var - e clamped at 0), plus its rounding.

   Every bound handed out is MARGIN = 2 times the derivation (the order of the additions within a lane is not pinned
   on the device: an unrolled loop may keep several partial sums) and times SLACK for the second-order terms.
   None of these numbers comes from what a device printed.

Elementwise bounds (forward value, dyh, column sums, dy) are counted the same way in `fwd_bound` / `bwd_bounds`; the
count is written next to each term there."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -150           # half the spacing of the fp32 subnormals: the absolute floor of one rounding
SLACK = 1.0 + 1e-5
MARGIN = 2.0
C_MEAN = 2
C_SQ = 3
# (row lanes, additions across the lanes) of the three statistics kernels: 64 x 4 scalar block (4 lane sums added to 0),
# 16 quads x 16 lanes float4 block, 32 x 32 short-matrix block (one cross-lane add, then 16 wave partials added to 0)
FORMS = {"scalar": (4, 4), "v4": (16, 16), "small": (32, 17)}

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3, 4
# sigmoid = 1 / (1 + exp(-v)) with the hardware exponential (1 ulp = 2 U, and the argument's scaling by log2 e rounds
# once: |v| U relative in the result); tanh from the device math library, held to the OpenCL full-profile limit of 5 ulp
EXP_ULP = 1.0
TANH_ULP = 5.0

FAMILIES = "abcdef"


# ================================================================================================== data families
def family_matrix(rows, c, chunk_rows, seed, fams=FAMILIES):
    """[rows x c] float32, column j of family fams[j % len(fams)]; returns (x, family letter per column).
    a N(0, 1); b constant 3.25; c mean 1e4, standard deviation 0.1; d N(0, 1) with the first row of every chunk at
    1e4; e +1 / -1 alternating down the rows; f magnitude 1e17."""
    rng = np.random.default_rng(seed)
    x = np.empty((rows, c), np.float32)
    fam = np.array([fams[j % len(fams)] for j in range(c)])
    r = np.arange(rows)
    for j in range(c):
        g = rng.standard_normal(rows)
        if fam[j] == "a":
            col = g
        elif fam[j] == "b":
            col = np.full(rows, 3.25)
        elif fam[j] == "c":
            col = 1e4 + 0.1 * g
        elif fam[j] == "d":
            col = g.copy()
            col[::chunk_rows] = 1e4
        elif fam[j] == "e":
            col = np.where(r % 2 == 0, 1.0, -1.0)
        else:
            col = 1e17 * g
        x[:, j] = col.astype(np.float32)
    return x, fam


def chunk_sizes(rows, chunk_rows):
    n = (rows + chunk_rows - 1) // chunk_rows
    return np.array([min(rows, (k + 1) * chunk_rows) - k * chunk_rows for k in range(n)], np.int64)


def sums_exact(rows, chunk_rows):
    """Family e (+-1 alternating) is exact through the fp32 chunk sums when every chunk has a power-of-two row count:
    d is 0 or -+2, the sums are small integers, and the division by n is exact too."""
    ns = chunk_sizes(rows, chunk_rows)
    return bool(np.all((ns & (ns - 1)) == 0))


# ==================================================================================================== definitions
def stats_def(x):
    """(mean, M2, var) of the columns of x in float64; M2 = sum (x - mean)^2, var = M2 / rows (biased)."""
    x = np.asarray(x, np.float64)
    mean = x.sum(0) / x.shape[0]
    m2 = ((x - mean) ** 2).sum(0)
    return mean, m2, m2 / x.shape[0]


def partials_def(x, chunk_rows):
    """Per chunk (mean_k, M2_k) in float64: [n_chunks x c] each."""
    x = np.asarray(x, np.float64)
    ns = chunk_sizes(x.shape[0], chunk_rows)
    mk = np.empty((len(ns), x.shape[1]))
    qk = np.empty_like(mk)
    for k in range(len(ns)):
        mk[k], qk[k], _ = stats_def(x[k * chunk_rows:k * chunk_rows + ns[k]])
    return mk, qk


def finish_def(mean, m2, n, eps, mm0=None, mv0=None, decay=0.0):
    """rstd and the moving averages from (mean, M2, n) in float64.  eps and decay are the float32 values the kernels
    receive.  Returns a dict of float64 arrays (round with F32 to compare bits)."""
    eps64, dec = float(F32(eps)), float(F32(decay))
    var = m2 / n
    out = {"mean": mean, "rstd": 1.0 / np.sqrt(var + eps64), "var": var}
    if mm0 is not None:
        unbiased = m2 / (n - 1) if n > 1 else var
        out["mm"] = np.asarray(mm0, np.float64) * dec + mean * (1.0 - dec)
        out["mv"] = np.asarray(mv0, np.float64) * dec + unbiased * (1.0 - dec)
    return out


def act_def(v, act, alpha):
    a = float(F32(alpha))
    if act == ACT_LRELU:
        return np.where(v > 0, v, v * a)
    if act == ACT_RELU:
        return np.where(v > 0, v, 0.0)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    if act == ACT_TANH:
        return np.tanh(v)
    return v


def act_grad_def(v, act, alpha):
    """Derivative from the activation's input; at 0 the leaky ReLU has slope alpha and the ReLU slope 0."""
    a = float(F32(alpha))
    if act == ACT_LRELU:
        return np.where(v > 0, 1.0, a)
    if act == ACT_RELU:
        return np.where(v > 0, 1.0, 0.0)
    if act == ACT_SIGMOID:
        s = 1.0 / (1.0 + np.exp(-v))
        return s * (1.0 - s)
    if act == ACT_TANH:
        t = np.tanh(v)
        return 1.0 - t * t
    return np.ones_like(v)


def _w(a):
    return None if a is None else np.asarray(a, np.float64)


def pre_def(y, mean, rstd, beta):
    if mean is None:                                   # a layer without batch norm: pre = xhat = y
        return _w(y), _w(y)
    xhat = (_w(y) - _w(mean)) * _w(rstd)
    return xhat, xhat + _w(beta)


def fwd_def(y, mean, rstd, beta, act, alpha, mask=None, res=()):
    _, pre = pre_def(y, mean, rstd, beta)
    z = act_def(pre, act, alpha)
    if mask is not None:
        z = z * _w(mask)
    for r in res:
        z = z + _w(r)
    return z


def fwd_f32(y, mean, rstd, beta, act, alpha):
    """fl(fl(fl(y - mean) * rstd) + beta), then the activation, every step one float32 operation: what common.h
    promises for activation none / leaky ReLU / ReLU without mask and residuals, bit for bit."""
    y, mean, rstd, beta = (np.asarray(a, np.float32) for a in (y, mean, rstd, beta))
    pre = ((y - mean).astype(np.float32) * rstd).astype(np.float32) + beta
    pre = pre.astype(np.float32)
    if act == ACT_LRELU:
        return np.where(pre > 0, pre, (pre * F32(alpha)).astype(np.float32)).astype(np.float32)
    if act == ACT_RELU:
        return np.where(pre > 0, pre, F32(0.0)).astype(np.float32)
    assert act == ACT_NONE
    return pre


def bwd_def(dz, y, mean, rstd, beta, act, alpha, mask=None, stat_rows=None, sums=None):
    """dict(dyh, xhat, s0, s1, dy).  sums: (s0, s1) to use instead of this matrix's own (the global-batch form).
    mean None (with rstd and beta): a layer without batch norm, pre = xhat = y and dy = dyh (hypel_act_bias_bwd_reduce)."""
    xhat, pre = pre_def(y, mean, rstd, beta)
    g = _w(dz) if mask is None else _w(dz) * _w(mask)
    dyh = g * act_grad_def(pre, act, alpha)
    s0, s1 = dyh.sum(0), (dyh * xhat).sum(0)
    n = float(y.shape[0] if stat_rows is None else stat_rows)
    u0, u1 = (s0, s1) if sums is None else (_w(sums[0]), _w(sums[1]))
    dy = dyh if mean is None else _w(rstd) * (dyh - u0 / n - xhat * u1 / n)   # no statistics: dy = dyh
    return {"dyh": dyh, "xhat": xhat, "pre": pre, "s0": s0, "s1": s1, "dy": dy}


# ====================================================================================================== fp32 twins
def _lane_sums(v, lanes):
    """float32 sum of the rows of v [n x c]: down each of `lanes` row lanes serially, then across the lanes from 0."""
    n, c = v.shape
    acc = np.zeros((lanes, c), np.float32)
    for i in range(0, n, lanes):
        blk = v[i:i + lanes]
        acc[:blk.shape[0]] = acc[:blk.shape[0]] + blk
    t = np.zeros(c, np.float32)
    for k in range(lanes):
        t = t + acc[k]
    return t


def _chunks(x, chunk_rows):
    ns = chunk_sizes(x.shape[0], chunk_rows)
    for k, n in enumerate(ns):
        yield k, int(n), x[k * chunk_rows:k * chunk_rows + n]


def twin_partials(x, chunk_rows, lanes):
    x = np.asarray(x, np.float32)
    ns = chunk_sizes(x.shape[0], chunk_rows)
    mk = np.empty((len(ns), x.shape[1]), np.float32)
    qk = np.empty_like(mk)
    with np.errstate(all="ignore"):
        for k, n, blk in _chunks(x, chunk_rows):
            d = blk - blk[0]
            ts, tss = _lane_sums(d, lanes), _lane_sums(d * d, lanes)
            mean_d = ts / F32(n)
            m2 = tss - ts * mean_d
            mk[k] = blk[0] + mean_d
            qk[k] = np.where(m2 < 0, F32(0), m2)
    return mk, qk


def naive_partials_sumsq(x, chunk_rows, lanes):
    """Naive twin 1: mean = sum x / n, M2 = sum x^2 - n mean^2, all in float32."""
    x = np.asarray(x, np.float32)
    ns = chunk_sizes(x.shape[0], chunk_rows)
    mk = np.empty((len(ns), x.shape[1]), np.float32)
    qk = np.empty_like(mk)
    with np.errstate(all="ignore"):
        for k, n, blk in _chunks(x, chunk_rows):
            ts, tss = _lane_sums(blk, lanes), _lane_sums(blk * blk, lanes)
            mk[k] = ts / F32(n)
            m2 = tss - ts * mk[k]
            qk[k] = np.where(m2 < 0, F32(0), m2)
    return mk, qk


def naive_partials_unshifted(x, chunk_rows, lanes):
    """Naive twin 2: the mean from an unshifted float32 sum, M2 from float32 deviations from that mean."""
    x = np.asarray(x, np.float32)
    ns = chunk_sizes(x.shape[0], chunk_rows)
    mk = np.empty((len(ns), x.shape[1]), np.float32)
    qk = np.empty_like(mk)
    with np.errstate(all="ignore"):
        for k, n, blk in _chunks(x, chunk_rows):
            mk[k] = _lane_sums(blk, lanes) / F32(n)
            d = blk - mk[k]
            qk[k] = _lane_sums(d * d, lanes)
    return mk, qk


def merge64(mk, qk, n_k):
    """Float64 merge of records (n_k, mean_k, M2_k) -> (mean, M2): deviations from the first record's mean."""
    mk, qk, n_k = np.asarray(mk, np.float64), np.asarray(qk, np.float64), np.asarray(n_k, np.float64)[:, None]
    with np.errstate(all="ignore"):
        n = n_k.sum()
        d = mk - mk[0]
        s = (n_k * d).sum(0)
        m2 = (qk + n_k * d * d).sum(0) - s * s / n
        return mk[0] + s / n, np.where(m2 < 0, 0.0, m2)


def naive_merge32(mk, qk, n_k):
    """Naive twin 3: the records merged with float32 running sums, record after record, in the textbook one-pass form
    mean = sum n_k mean_k / N, M2 = sum (M2_k + n_k mean_k^2) - N mean^2.  (A float32 merge that first forms the mean
    and then sums deviations from it stays inside the bounds at a few hundred records: what the float64 step buys is
    doing it in ONE pass over the records.)"""
    mk, qk = np.asarray(mk, np.float32), np.asarray(qk, np.float32)
    n = F32(np.sum(n_k))
    s = np.zeros(mk.shape[1], np.float32)
    t = np.zeros(mk.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for k in range(len(n_k)):
            s = s + F32(n_k[k]) * mk[k]
            t = t + (qk[k] + F32(n_k[k]) * mk[k] * mk[k])
        mean = s / n
        m2 = t - n * mean * mean
    return mean.astype(np.float64), np.where(m2 < 0, 0.0, m2.astype(np.float64))


# ========================================================================================================== bounds
def chain(n, form):
    lanes, cross = FORMS[form]
    return -(-int(n) // lanes) + cross


def rnd(v):
    """One rounding to float32 of the value v."""
    return U * np.abs(v) + TINY


def partial_bounds(x, chunk_rows, form):
    """Derived bounds (before MARGIN) on every chunk record: (e_mean_k, e_m2_k), [n_chunks x c] float64."""
    x = np.asarray(x, np.float64)
    mk, qk = partials_def(x, chunk_rows)
    em, eq = np.empty_like(mk), np.empty_like(mk)
    for k, n, blk in _chunks(x, chunk_rows):
        d = blk - blk[0]
        s, a, d2 = np.abs(d.sum(0)), np.abs(d).sum(0), (d * d).sum(0)
        ln = chain(n, form)
        em[k] = (ln + C_MEAN) * U * a / n + rnd(mk[k])
        eq[k] = (ln + C_SQ) * U * d2 + 2 * (ln + C_MEAN) * U * s * a / n + rnd(qk[k])
    return em, eq


def merge_bounds(n_k, mk, em, eq):
    """Bounds (before MARGIN) on the float64 merge of records whose means / M2 are off by at most em / eq."""
    n_k = np.asarray(n_k, np.float64)[:, None]
    n = n_k.sum()
    mean = (n_k * mk).sum(0) / n
    e_mean = (n_k * em).sum(0) / n
    g = em + e_mean
    e_m2 = eq.sum(0) + (n_k * (2 * np.abs(mk - mean) * g + g * g)).sum(0)
    return e_mean, e_m2


def rstd_bound(m2, e_m2, n, eps):
    """Largest one-sided change of 1 / sqrt(M2 / n + eps) over M2 +- e_m2 (clamped at 0), plus its fp32 rounding."""
    eps64 = float(F32(eps))
    r = 1.0 / np.sqrt(m2 / n + eps64)
    lo = 1.0 / np.sqrt((m2 + e_m2) / n + eps64)
    hi = 1.0 / np.sqrt(np.maximum(m2 - e_m2, 0.0) / n + eps64)
    return np.maximum(r - lo, hi - r) + rnd(r)


def stats_bounds(x, chunk_rows, form, eps, decay=0.0):
    """Everything a statistics test needs for ONE matrix, bounds already times MARGIN * SLACK:
    dict(part_mean, part_m2 [n_chunks x c], mean, m2, rstd, mm, mv [c]); m2 is for a float32-stored merged M2."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    ns = chunk_sizes(n, chunk_rows)
    mk, _ = partials_def(x, chunk_rows)
    em, eq = partial_bounds(x, chunk_rows, form)
    e_mean, e_m2 = merge_bounds(ns, mk, em, eq)
    mean, m2, var = stats_def(x)
    dec = float(F32(decay))
    unb_n = n - 1 if n > 1 else n
    k = MARGIN * SLACK
    # the moving averages: (1 - decay) times the statistic's error, plus the rounding of the stored result, which is at
    # most |old| decay + |statistic| (1 - decay) in size
    return {"part_mean": k * em, "part_m2": k * eq, "mean": k * (e_mean + rnd(mean)), "m2": k * (e_m2 + rnd(m2)),
            "rstd": k * rstd_bound(m2, e_m2, n, eps), "raw_mean": e_mean, "raw_m2": e_m2,
            "mm_gain": k * (1 - dec) * e_mean, "mv_gain": k * (1 - dec) * e_m2 / unb_n}


def moving_bounds(sb, mm_def, mv_def):
    """Bounds on the stored moving averages given stats_bounds() and their float64 definitions."""
    k = MARGIN * SLACK
    return sb["mm_gain"] + k * rnd(mm_def), sb["mv_gain"] + k * rnd(mv_def)


def _act_bounds(pre, e_pre, act, alpha):
    """(error of act(pre), error of act'(pre)) for a device pre within e_pre of the float64 `pre`."""
    a = float(F32(alpha))
    val = act_def(pre, act, alpha)
    near = np.abs(pre) <= e_pre                        # the device may sit on the other side of the kink
    if act == ACT_NONE:
        return e_pre, np.zeros_like(pre)
    if act == ACT_LRELU:                               # Lipschitz 1, one product; the slope jumps by 1 - alpha
        return e_pre + rnd(val), np.where(near, 1.0 - a, 0.0)
    if act == ACT_RELU:
        return e_pre, np.where(near, 1.0, 0.0)
    if act == ACT_SIGMOID:
        # e = exp(-v): (2 EXP_ULP + 1.5 |v|) U relative (1.5 > log2 e: the scaled argument's rounding); s = 1 / (1 + e):
        # ds / s = (1 - s) de / e, one addition, one division; Lipschitz 1/4 for the value and 1/10 for s (1 - s)
        es = val * ((1 - val) * (2 * EXP_ULP + 1.5 * np.abs(pre)) + 2) * U
        return e_pre / 4 + es, e_pre / 10 + es + 2 * U * val * (1 - val)
    # tanh: Lipschitz 1, TANH_ULP ulps; 1 - t^2: 2 |t| dt, a product and a subtraction (each <= U in absolute size)
    et = e_pre + 2 * TANH_ULP * U * np.abs(val) + TINY
    return et, 2 * np.abs(val) * et + 2 * U


def pre_bound(y, mean, rstd, beta):
    """xhat = fl(fl(y - mean) * rstd): 2 U |xhat|; pre = fl(xhat + beta): one more rounding."""
    xhat, pre = pre_def(y, mean, rstd, beta)
    if mean is None:                                   # pre = xhat = y, an input: no rounding
        return np.zeros_like(xhat), np.zeros_like(xhat)
    e_x = 2 * U * np.abs(xhat) + TINY
    return e_x, e_x + rnd(pre)


def fwd_bound(y, mean, rstd, beta, act, alpha, mask=None, res=()):
    """Bound (times MARGIN) on z = act(pre) * mask + res1 + res2: the activation's error times |mask|, one rounding for
    the product with the mask, one per residual addition (each of the size of the running value)."""
    _, pre = pre_def(y, mean, rstd, beta)
    _, e_pre = pre_bound(y, mean, rstd, beta)
    e, _ = _act_bounds(pre, e_pre, act, alpha)
    z = act_def(pre, act, alpha)
    if mask is not None:
        z = z * _w(mask)
        e = e * np.abs(_w(mask)) + rnd(z)
    for r in res:
        z = z + _w(r)
        e = e + rnd(z)
    return MARGIN * SLACK * e


def bwd_bounds(dz, y, mean, rstd, beta, act, alpha, mask, chunk_rows, form, stat_rows=None, sums=None, e_sums=None):
    """Bounds (times MARGIN) dict(s0, s1, dy) for the backward chain.
      dyh = fl(fl(dz mask) act'):  |dz mask| times the derivative's error, plus 2 U |dyh|
      s0: every dyh's error, plus (L + 1) U sum |dyh| (L float32 additions within a chunk, the float64 merge of the
          chunks, one rounding of the stored sum);  s1 the same over dyh xhat, whose terms carry dyh's error times
          |xhat|, xhat's error times |dyh| and the product's rounding
      dy = fl(rstd fl(fl(dyh - m0) - fl(xhat m1))), m0 = fl(s0 fl(1 / N)), m1 likewise: (e_s + 2 U |s|) / N each, the
          product xhat m1 (xhat's error, m1's error, one rounding), two subtractions of values no larger than
          |dyh| + |m0| + |xhat m1|, and the final product's U |dy|.
    sums / e_sums: externally supplied (s0, s1) that are exact inputs (e_sums None) or carry the given errors."""
    d = bwd_def(dz, y, mean, rstd, beta, act, alpha, mask, stat_rows, sums)
    e_x, e_pre = pre_bound(y, mean, rstd, beta)
    _, e_g = _act_bounds(d["pre"], e_pre, act, alpha)
    g = np.abs(_w(dz) if mask is None else _w(dz) * _w(mask))
    dyh, xhat = d["dyh"], d["xhat"]
    e_dyh = g * e_g + 2 * U * np.abs(dyh) + TINY
    t1 = dyh * xhat
    e_t1 = e_dyh * np.abs(xhat) + np.abs(dyh) * e_x + rnd(t1)
    rows = y.shape[0]
    ln = chain(min(chunk_rows, rows), form) + 1
    e_s0 = e_dyh.sum(0) + ln * U * np.abs(dyh).sum(0)
    e_s1 = e_t1.sum(0) + ln * U * np.abs(t1).sum(0)
    n = float(rows if stat_rows is None else stat_rows)
    if sums is None:
        u0, u1, f0, f1 = d["s0"], d["s1"], e_s0, e_s1
    else:
        u0, u1 = _w(sums[0]), _w(sums[1])
        f0, f1 = (0.0, 0.0) if e_sums is None else e_sums
    m0, m1 = u0 / n, u1 / n
    e_m0, e_m1 = (f0 + 2 * U * np.abs(u0)) / n, (f1 + 2 * U * np.abs(u1)) / n
    xm = xhat * m1
    inner = (e_dyh + e_m0 + np.abs(xhat) * e_m1 + np.abs(m1) * e_x + rnd(xm)
             + 2 * U * (np.abs(dyh) + np.abs(m0) + np.abs(xm)))
    e_dy = e_dyh if mean is None else np.abs(_w(rstd)) * inner + rnd(d["dy"])   # no statistics: dy = dyh
    k = MARGIN * SLACK
    return {"s0": k * e_s0, "s1": k * e_s1, "dy": k * e_dy, "def": d}
