"""-m gpu: the small kernels at the end of a training step (csrc/elementwise.hip) -- dropout bits, loss finaliser and
guard, guarded optimiser updates, softmax cross entropy at large logits, fill, rstd -- each against a plain definition
of the same operation in higher precision (float64 NumPy, oracle/train.py, tests/philox_ref.py), through the C-ABI.

Every tolerance here is one of two kinds: derived in the docstring of its test from a count of fp32 roundings (in
units of U = 2^-24, half an fp32 ulp relative to the magnitude named there) or from a stated probability; or measured
against float64 and written down with the measurement, the margin and the reason (the device expf / logf figures of the
softmax test).  None is taken from what the kernel under test produced."""
import functools
import math

import numpy as np
import pytest

from hypelcnn_amd.backend import Ref
from oracle import train as oracle_train
from tests import philox_ref as P

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # unit roundoff of fp32: one rounding moves a value by at most U * |value| (half an ulp)
TINY = 2.0 ** -150        # half the spacing of the fp32 subnormals: the absolute floor of one rounding
SLACK = 1.0 + 1e-6        # second-order terms (U^2) and the float64 reference's own rounding (2^-53)
SENT = np.float32(-12345.5)
F32 = np.float32


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


def _host(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bit(x):
    return int(np.float32(x).view(np.uint32))


def _ordered(a):
    """fp32 -> integers monotone in the value (+-0 both 0): a difference of 1 is one ulp."""
    b = _bits(a).astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7FFFFFFF), b)


def _ulps(a, b):
    return np.abs(_ordered(a) - _ordered(b))


def _u64(hip, value):
    return hip.upload(np.array([int(value)], np.uint64).view(np.int64))


def _read_u64(t):
    return int(_host(t).view(np.uint64)[0])


# ============================================================================================== dropout: the bits
S_LAYER = P.layer_seed(1234, 3)                 # 1234 * 1000003 + 3: single process, fits 32 bits + a little
S_RANK7 = P.layer_seed(1234, 3, rank=7)         # rank 7 of the product's own formula: high key word live
S_ALL = 2 ** 64 - 1
SEEDS = [S_LAYER, S_RANK7, S_ALL]
STEPS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7]
COUNTS = [1, 3, 4, 5, 1023, 4097, 2 ** 21 + 5]   # 2^21 + 5: first count whose groups exceed 2048 blocks x 256 threads
DROPOUT_CASES = ([(n, 0.3, S_RANK7, 2 ** 40 + 7) for n in COUNTS]
                 + [(4097, keep, seed, step) for keep in (0.3, 0.5, 0.7, 1.0) for seed in SEEDS for step in STEPS]
                 + [(2 ** 21 + 5, 1.0, S_ALL, 2 ** 32), (2 ** 21 + 5, 0.7, S_LAYER, 2 ** 32 - 1), (5, 0.5, S_ALL, 0),
                    (3, 0.7, S_LAYER, 1)])


def _run_mask(hip, count, keep, seed, step_t):
    buf = hip.upload(np.full(count + 8, SENT, np.float32))
    hip.call("dropout_mask", Ref(buf), count, float(keep), int(seed), Ref(step_t))
    got = _host(buf)
    assert np.array_equal(_bits(got[count:]), _bits(np.full(8, SENT))), "wrote past count"
    return got[:count]


def _check_mask(got, count, keep, seed, step):
    """Zero / non-zero pattern bit for bit; kept elements all hold ONE value, within 1 ulp of fp32 1 / keep (the
    kernel's own division is a single correctly rounded fp32 operation: 1 ulp allows a reciprocal instruction)."""
    want = P.mask_reference(count, keep, seed, step)
    kept = got != 0.0
    bad = np.flatnonzero(kept != want)
    assert bad.size == 0, f"{bad.size} of {count} elements differ from Philox4x32-10, first at {bad[:8]}"
    vals = np.unique(_bits(got[kept]))
    assert vals.size <= 1, f"kept elements hold {vals.size} distinct values"
    if vals.size:
        assert _ulps(vals.view(np.float32), F32(1.0) / F32(keep))[0] <= 1
    assert np.array_equal(_bits(got[~kept]), np.zeros(int((~kept).sum()), np.uint32)), "dropped elements are +0"


@pytest.mark.parametrize("count,keep,seed,step", DROPOUT_CASES)
def test_dropout_mask_is_philox4x32_10_bit_for_bit(hip, count, keep, seed, step):
    got = _run_mask(hip, count, keep, seed, _u64(hip, step))
    _check_mask(got, count, keep, seed, step)
    if keep == 1.0:
        assert (got == 1.0).all()


def test_dropout_keeps_strictly_below_keep(hip):
    """u takes multiples of 2^-24, so u == keep happens once in 2^24 draws: no random case meets it.  Take keep FROM the
    reference's own draw of one element: that element has u == keep exactly and is dropped (`<`, not `<=`)."""
    count, seed, step = 4097, S_RANK7, 2 ** 32
    w = P.uniform_words(count, seed, step)
    u = (w >> np.uint32(8)).astype(np.float32) * F32(2.0 ** -24)
    i = int(np.flatnonzero((u > 0.2) & (u < 0.8))[0])
    keep = float(u[i])
    got = _run_mask(hip, count, keep, seed, _u64(hip, step))
    assert got[i] == 0.0, "the element whose draw equals keep is dropped"
    _check_mask(got, count, keep, seed, step)


def test_step_counter_carries_into_the_high_word(hip):
    step_t = _u64(hip, 2 ** 32 - 1)
    hip.call("step_inc", Ref(step_t))
    assert _read_u64(step_t) == 2 ** 32
    got = _run_mask(hip, 4097, 0.3, S_RANK7, step_t)
    _check_mask(got, 4097, 0.3, S_RANK7, 2 ** 32)
    assert _read_u64(step_t) == 2 ** 32, "the mask kernel only reads the counter"


def test_dropout_streams_of_the_product_are_independent(hip):
    """Layers idx / idx+1, steps s / s+1 and ranks r / r+1, with the seeds as plan.py and runtime._rank_seed form them.
    Independent Bernoulli(p) masks agree at an element with probability a = p^2 + (1-p)^2; over n = 2^20 elements the
    rate has standard deviation sqrt(a(1-a)/n) <= 4.9e-4, so |rate - a| <= 3e-3 is six sigma (derived; the CPU test
    test_philox_ref.py shows mask_reference alone meets it for these exact seeds)."""
    n, keep = P.INDEP_N, P.INDEP_KEEP
    a = P.independent_agreement(keep)
    for name, (s0, t0), (s1, t1) in P.INDEP_PAIRS:
        m0 = _run_mask(hip, n, keep, s0, _u64(hip, t0)) != 0.0
        m1 = _run_mask(hip, n, keep, s1, _u64(hip, t1)) != 0.0
        rate = float((m0 == m1).mean())
        print(f"{name}: agreement {rate:.6f} (independent: {a:.6f})")
        assert abs(rate - a) <= P.INDEP_BOUND, name


# ================================================================================================ loss guard
@pytest.mark.parametrize("a,b,want", [
    (1.5, None, 0.0), (1.5, 2.5, 0.0), (np.nan, None, 1.0), (np.inf, None, 1.0), (-np.inf, 2.5, 1.0), (1.5, np.nan, 1.0),
    (1.5, np.inf, 1.0), (3.4e38, 3.4e38, 0.0)])
def test_loss_guard_verdicts(hip, a, b, want):
    """The flag sits between two sentinels (in production the element before it is the last gradient) and starts as
    the opposite of the expected verdict; only flag[0] may change."""
    ab = hip.upload(np.array([a, 0.0 if b is None else b], np.float32))
    start = np.array([SENT, 1.0 - want, SENT], np.float32)
    buf = hip.upload(start)
    hip.call("loss_guard_f32", Ref(ab, 0), None if b is None else Ref(ab, 1), Ref(buf, 1))
    got = _host(buf)
    assert _bits(got)[1] == _bit(F32(want)), f"flag {got[1]} for ({a}, {b})"
    assert np.array_equal(_bits(got[[0, 2]]), _bits(start[[0, 2]])), "neighbours of the flag"
    assert np.array_equal(_bits(_host(ab)), _bits(np.array([a, 0.0 if b is None else b], np.float32)))


# ======================================================================================== guarded optimisers
OPT_COUNTS = [0, 1, 255, 257, 524288 + 257]  # 2048 blocks x 256 threads = 524288: the last takes a second grid sweep
TAIL = 4
B1, B2, EPS = F32(0.9), F32(0.999), F32(1e-8)
ADAM_T = 7
# lr such that the oracle's lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t) IS the fp32 lr_t the kernel receives (to 2^-53)
LR_T = F32(3e-4 * math.sqrt(1 - 0.999 ** ADAM_T) / (1 - 0.9 ** ADAM_T))
MOM_LR, MOM_MU = F32(1e-3), F32(0.9)


def _adam_oracle_lr():
    b1, b2 = float(B1), float(B2)
    return float(LR_T) / (math.sqrt(1 - b2 ** ADAM_T) / (1 - b1 ** ADAM_T))


@functools.lru_cache(maxsize=None)
def _opt_inputs(count):
    """p over six decades (so that the update is not everywhere hidden below half an ulp of p), g, m of either sign
    (so that b1 * m + (1 - b1) * g cancels somewhere), v >= 0.  Read-only: every run uploads copies."""
    rng = np.random.default_rng(500 + count)
    n = count + TAIL
    d = {"p": (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32),
         "g": rng.standard_normal(n).astype(np.float32),
         "m": rng.standard_normal(n).astype(np.float32),
         "v": rng.random(n).astype(np.float32)}
    for a in d.values():
        a.setflags(write=False)
    return d


def _run_opt(hip, opt, count, skip="unguarded", inputs=None):
    """One launch on fresh copies (count elements + TAIL elements behind them that no launch may touch).  skip:
    "unguarded" = the plain entry point, None = guarded with a NULL flag, a float = the flag's value."""
    src = inputs if inputs is not None else _opt_inputs(count)
    names = ("p", "m", "v") if opt == "adam" else ("p", "m")
    dev = {k: hip.upload(src[k]) for k in names + ("g",)}
    flag = None
    if skip != "unguarded" and skip is not None:
        flag_start = np.array([SENT, skip, SENT], np.float32)
        flag = hip.upload(flag_start)
    sref = None if flag is None else Ref(flag, 1)
    if opt == "adam":
        args = [Ref(dev["p"]), Ref(dev["g"]), Ref(dev["m"]), Ref(dev["v"]), count, float(LR_T), float(B1), float(B2),
                float(EPS)]
    else:
        args = [Ref(dev["p"]), Ref(dev["g"]), Ref(dev["m"]), count, float(MOM_LR), float(MOM_MU)]
    if skip == "unguarded":
        hip.call(opt + "_tf1", *args)
    else:
        hip.call(opt + "_tf1_guarded", *args, sref)
    out = {k: _host(dev[k]) for k in names}
    assert np.array_equal(_bits(_host(dev["g"])), _bits(src["g"])), "the gradient is an input"
    if flag is not None:
        assert np.array_equal(_bits(_host(flag)), _bits(flag_start)), "the flag is an input"
    for k in names:
        assert np.array_equal(_bits(out[k][count:]), _bits(src[k][count:])), f"{k}: wrote past count"
    return out


@pytest.mark.parametrize("count", OPT_COUNTS)
@pytest.mark.parametrize("opt", ["adam", "momentum"])
def test_guarded_optimisers_apply_or_refuse(hip, opt, count):
    """skip NULL / +0 / -0: bit-identical to the unguarded entry point (-0.0 == 0 under `!= 0`: the update is applied;
    this records the current meaning).  skip 1 (one rank), 2 and 8 (the flag summed over ranks), NaN and +inf (a NaN that
    reached the flag): parameters and slots bitwise unchanged.  For momentum the accumulator `a` is stored under "m"."""
    src = _opt_inputs(count)
    base = _run_opt(hip, opt, count)
    if count:
        for k in base:
            assert not np.array_equal(_bits(base[k][:count]), _bits(src[k][:count])), f"{k}: the update is applied"
    for skip in (None, 0.0, -0.0):
        got = _run_opt(hip, opt, count, skip)
        for k in base:
            assert np.array_equal(_bits(got[k]), _bits(base[k])), f"{k} with skip={skip!r}"
    for skip in (1.0, 2.0, 8.0, np.nan, np.inf):
        got = _run_opt(hip, opt, count, skip)
        for k in base:
            assert np.array_equal(_bits(got[k]), _bits(src[k])), f"{k} changed although skip={skip!r}"


def _report(name, err, bound):
    """Print the worst ratio error / bound; on failure say by how much (never loosen silently)."""
    ratio = err / bound
    i = int(np.argmax(ratio))
    print(f"{name}: worst error / bound = {ratio[i]:.3f} at element {i}")
    assert ratio[i] <= 1.0, f"{name}: element {i} exceeds its derived bound by a factor {ratio[i]:.3f}"


@pytest.mark.parametrize("count", [c for c in OPT_COUNTS if c])
def test_adam_tf1_against_float64(hip, count):
    """oracle/train.py adam_tf1_step on float64 copies of the same fp32 inputs (beta, eps, lr_t as the fp32 values the
    kernel receives).  Roundings of the kernel, each at most U = 2^-24 of the magnitude it acts on; a fused
    multiply-add only removes one.  1 - beta is formed in fp32 but is EXACT for beta in [0.5, 1] (Sterbenz), asserted
    below, so it costs nothing.

    m = b1*m + (1-b1)*g: two products and a sum = 3 roundings, each of a quantity no larger than
        S = |b1*m| + |(1-b1)*g| (the terms may cancel, so S and not |m_new| is the magnitude):     |dm| <= 3 U S
    v = b2*v + ((1-b2)*g)*g: two roundings on the small term, one on b2*v, one on the sum; the terms are >= 0, so
        |dv| <= U (b2 v + 2 (1-b2) g^2 + v_new) <= 3 U v_new                                        -- 3 half-ulps of |v|
    p = p - (lr_t*m) / (sqrt(v) + eps), with D = lr_t * S / (sqrt(v) + eps) >= |update|: inherited 3 U D from m and
        1.5 U D from v (through the square root), then a square root, a sum, a product and a quotient (4 U D) and the
        difference (U |p_new|):                                                |dp| <= U (|p_new| + 8.5 D)
        which is within 9.5 half-ulps of max(|p_new|, D); the split form asserted here is the tighter of the two."""
    src = _opt_inputs(count)
    got = _run_opt(hip, "adam", count)
    b1, b2, eps = float(B1), float(B2), float(EPS)
    assert float(F32(1) - B1) == 1.0 - b1 and float(F32(1) - B2) == 1.0 - b2, "1 - beta is exact in fp32"
    p, g, m, v = (src[k][:count].astype(np.float64) for k in ("p", "g", "m", "v"))
    s_abs = np.abs(b1 * m) + np.abs((1 - b1) * g)
    oracle_train.adam_tf1_step(p, g, m, v, _adam_oracle_lr(), ADAM_T, beta1=b1, beta2=b2, eps=eps)
    d_abs = float(LR_T) * s_abs / (np.sqrt(v) + eps)
    _report("adam m", np.abs(got["m"][:count] - m), (3 * U * s_abs + 3 * TINY) * SLACK)
    _report("adam v", np.abs(got["v"][:count] - v), (3 * U * v + 4 * TINY) * SLACK)
    _report("adam p", np.abs(got["p"][:count] - p), (U * (np.abs(p) + 8.5 * d_abs) + 6 * TINY) * SLACK)


@pytest.mark.parametrize("count", [c for c in OPT_COUNTS if c])
def test_momentum_tf1_against_float64(hip, count):
    """oracle/train.py momentum_tf1_step in float64.  a = mu*a + g: a product and a sum, S = |mu*a| + |g|:
    |da| <= 2 U S.  p = p - lr*a: inherited 2 U lr S, a product (U lr |a|) and the difference (U |p_new|):
    |dp| <= U (|p_new| + 3 lr S)."""
    src = _opt_inputs(count)
    got = _run_opt(hip, "momentum", count)
    lr, mu = float(MOM_LR), float(MOM_MU)
    p, g, a = (src[k][:count].astype(np.float64) for k in ("p", "g", "m"))
    s_abs = np.abs(mu * a) + np.abs(g)
    oracle_train.momentum_tf1_step(p, g, a, lr, mu)
    _report("momentum a", np.abs(got["m"][:count] - a), (2 * U * s_abs + 2 * TINY) * SLACK)
    _report("momentum p", np.abs(got["p"][:count] - p), (U * (np.abs(p) + 3 * lr * s_abs) + 4 * TINY) * SLACK)


def _fma(a, b, c):
    """fp32 fused multiply-add through float64: the product of two fp32 values is exact there; the one float64 rounding
    of the sum before the fp32 one could differ from a true fma only once in about 2^29 operands."""
    with np.errstate(all="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _one_of(name, got, unfused, *fused):
    """got equals the plain fp32 restatement bit for bit, or, element by element, one of the forms in which the
    compiler contracts a product and the sum into a fused multiply-add (legitimate: -ffp-contract is on for device
    code); those elements are printed, and are within 1 ulp of the plain form (no cancellation in these cases)."""
    plain = _bits(got) == _bits(unfused)
    ok = plain.copy()
    for f in fused:
        ok |= _bits(got) == _bits(f)
    if not plain.all():
        print(f"{name}: elements {np.flatnonzero(~plain).tolist()} follow a fused form "
              f"({got[~plain].tolist()} vs plain {unfused[~plain].tolist()})")
    assert ok.all(), f"{name}: elements {np.flatnonzero(~ok).tolist()}: {got[~ok]} vs {unfused[~ok]}"
    assert (_ulps(got, unfused) <= 1).all(), name


# edge elements (g, m, v); each is run with p = 0.5 and with p = 0
EDGE_GMV = [
    (0.0, 0.0, 0.0),          # nothing to do: the update is 0 / (0 + eps) = 0, no NaN
    (1e-40, 0.0, 0.0),        # subnormal gradient
    (-1e-40, 0.0, 0.0),
    (1e19, 0.0, 0.0),         # g^2 = 1e38 still finite
    (3e19, 0.0, 0.0),         # g*g alone would overflow; ((1-b2)*g)*g = 9e35 does not: the association matters
    (1e21, 0.0, 0.0),         # ((1-b2)*g)*g overflows: v = inf, update = m / inf = 0, p unchanged
    (1e-20, 1e-3, 1e-30),     # sqrt(v) = 1e-15 << eps: eps is the denominator
    (0.0, 1e-3, 1e-40),       # subnormal v
    (1e-3, 2e-3, 1e-30),
    (0.5, 0.25, 0.125),       # an ordinary element
]


def test_adam_tf1_edge_values(hip):
    """Against a NumPy float32 restatement, element by element and bit for bit (see _one_of for contraction).  p is
    compared with the restatement evaluated on the device's own new m and v -- themselves held bit for bit just
    before -- because p - (lr_t*m)/(sqrt(v)+eps) offers the compiler nothing to contract.  p finite everywhere."""
    g, m, v = (np.array([e[k] for e in EDGE_GMV] * 2, np.float32) for k in range(3))
    n = len(EDGE_GMV)
    p = np.array([0.5] * n + [0.0] * n, np.float32)
    pad = np.zeros(TAIL, np.float32)
    src = {"p": np.concatenate([p, pad]), "g": np.concatenate([g, pad]), "m": np.concatenate([m, pad]),
           "v": np.concatenate([v, pad])}
    got = {k: a[:2 * n] for k, a in _run_opt(hip, "adam", 2 * n, inputs=src).items()}
    with np.errstate(all="ignore"):
        c1g, c2gg = (F32(1) - B1) * g, ((F32(1) - B2) * g) * g
        _one_of("m", got["m"], B1 * m + c1g, _fma(np.full_like(m, B1), m, c1g), _fma(np.full_like(g, F32(1) - B1), g, B1 * m))
        _one_of("v", got["v"], B2 * v + c2gg, _fma(np.full_like(v, B2), v, c2gg), _fma((F32(1) - B2) * g, g, B2 * v))
        p_want = p - (LR_T * got["m"]) / (np.sqrt(got["v"]) + EPS)
    assert np.array_equal(_bits(got["p"]), _bits(p_want)), f"p: {got['p']} vs {p_want}"
    assert np.isfinite(got["p"]).all() and not np.isnan(got["m"]).any() and not np.isnan(got["v"]).any()
    for i in (0, n):  # g = m = v = 0: the update is exactly 0
        assert _bits(got["p"])[i] == _bits(p)[i] and got["m"][i] == 0.0 and got["v"][i] == 0.0
    for i in (4, n + 4):  # g = 3e19: finite v by association
        assert np.isfinite(got["v"][i]) and got["v"][i] > 8e35
    for i in (5, n + 5):  # g = 1e21: v = inf, the update is 0
        assert np.isinf(got["v"][i]) and _bits(got["p"])[i] == _bits(p)[i] and np.isfinite(got["m"][i])


def test_momentum_tf1_edge_values(hip):
    """The same gradients through a = mu*a + g, p = p - lr*a (a from the m column): bit for bit against the fp32
    restatement or its fused forms; p finite."""
    g, a = (np.array([e[k] for e in EDGE_GMV] * 2, np.float32) for k in range(2))
    n = len(EDGE_GMV)
    p = np.array([0.5] * n + [0.0] * n, np.float32)
    pad = np.zeros(TAIL, np.float32)
    src = {"p": np.concatenate([p, pad]), "g": np.concatenate([g, pad]), "m": np.concatenate([a, pad])}
    got = {k: x[:2 * n] for k, x in _run_opt(hip, "momentum", 2 * n, inputs=src).items()}
    with np.errstate(all="ignore"):
        _one_of("a", got["m"], MOM_MU * a + g, _fma(np.full_like(a, MOM_MU), a, g))
        _one_of("p", got["p"], p - MOM_LR * got["m"], _fma(np.full_like(a, -MOM_LR), got["m"], p))
    assert np.isfinite(got["p"]).all() and np.isfinite(got["m"]).all()
    for i in (0, n):
        assert _bits(got["p"])[i] == _bits(p)[i] and got["m"][i] == 0.0


# ============================================================================================ loss finaliser
N_MSE = 1024  # HYPEL_MSE_PARTIALS


def _finalize(hip, rows, mse=None, scale=0.0, with_flag=True, with_step=True, flag0=0.0, step0=41):
    """One launch; returns (ce, mse, flag, step), None where the argument was NULL.  Every output sits between
    sentinels that must survive."""
    rows_t = hip.upload(np.asarray(rows, np.float32))
    mse_t = None if mse is None else hip.upload(np.asarray(mse, np.float32))
    start = np.array([SENT, -1.0, SENT], np.float32)
    ce_t, out_mse_t = hip.upload(start), hip.upload(start)
    flag_t = hip.upload(np.array([SENT, flag0, SENT], np.float32))
    step_start = np.array([77, step0, 99], np.uint64)
    step_t = hip.upload(step_start.view(np.int64))
    hip.call("loss_finalize_f32", Ref(rows_t), len(rows), None if mse is None else Ref(mse_t), float(scale),
             Ref(ce_t, 1), None if mse is None else Ref(out_mse_t, 1), Ref(flag_t, 1) if with_flag else None,
             Ref(step_t, 1) if with_step else None)
    ce, om, fl, st = _host(ce_t), _host(out_mse_t), _host(flag_t), _host(step_t).view(np.uint64)
    for name, a in (("ce", ce), ("mse", om), ("flag", fl)):
        assert np.array_equal(_bits(a[[0, 2]]), _bits(start[[0, 2]])), f"neighbours of {name}"
    assert st[0] == 77 and st[2] == 99, "neighbours of the step counter"
    if mse is None:
        assert _bits(om)[1] == _bits(start)[1]
    if not with_flag:
        assert _bits(fl)[1] == _bit(F32(flag0))
    if not with_step:
        assert int(st[1]) == step0
    return ce[1], (om[1] if mse is not None else None), (fl[1] if with_flag else None), (int(st[1]) if with_step else None)


def _mean64(x):
    return math.fsum(float(t) for t in np.asarray(x, np.float32)) / len(x)


@pytest.mark.parametrize("n_rows", [1, 255, 256, 257, 1000])
def test_loss_finalize_flags_a_nonfinite_row_wherever_it_sits(hip, n_rows):
    """One NaN / +inf / -inf row at index 0, 255, 256 (either side of the 256-thread stride) and n_rows - 1, with and
    without a finite MSE term; the flag starts as 0."""
    rng = np.random.default_rng(n_rows)
    mse = rng.random(N_MSE).astype(np.float32)
    for idx in sorted({i for i in (0, 255, 256, n_rows - 1) if i < n_rows}):
        for bad in (np.nan, np.inf, -np.inf):
            rows = rng.random(n_rows).astype(np.float32)
            rows[idx] = bad
            for m in (None, mse):
                ce, om, flag, step = _finalize(hip, rows, m, 1.0 / N_MSE, flag0=0.0)
                assert flag == 1.0, f"row {idx} = {bad}, mse {'given' if m is not None else 'NULL'}"
                assert not np.isfinite(ce) and step == 42
                if m is not None:
                    assert abs(float(om) - _mean64(mse)) <= np.spacing(F32(_mean64(mse)))


@pytest.mark.parametrize("idx", [0, N_MSE - 1])
def test_loss_finalize_flags_a_nonfinite_mse_partial(hip, idx):
    """Finite rows, NaN in one MSE partial: flag 1, and out_ce is still the float64 mean rounded to fp32."""
    rng = np.random.default_rng(60 + idx)
    rows = (rng.random(1000) * 3).astype(np.float32)
    mse = rng.random(N_MSE).astype(np.float32)
    mse[idx] = np.nan
    ce, om, flag, step = _finalize(hip, rows, mse, 1.0 / N_MSE, flag0=0.0)
    assert flag == 1.0 and np.isnan(om) and step == 42
    assert _bit(ce) == _bit(_mean64(rows)), f"{ce} vs {_mean64(rows)}"


def test_loss_finalize_accumulates_in_fp64(hip):
    """1000 rows of 3.0e38: any fp32 partial sum of more than one row is inf, the float64 mean is finite.  Every float64
    partial sum of k <= 1000 equal fp32 values is exact (24 + 10 bits), and so is the division: out_ce is fp32(3.0e38)
    exactly, flag 0."""
    rows = np.full(1000, 3.0e38, np.float32)
    ce, _, flag, _ = _finalize(hip, rows, flag0=1.0)
    assert flag == 0.0 and _bit(ce) == _bit(F32(3.0e38)), ce


def test_loss_finalize_flags_an_mse_that_overflows_fp32(hip):
    """Finite partials whose float64 sum times mse_scale is beyond FLT_MAX: out_mse = inf, flag 1; out_ce is finite."""
    rows = np.full(10, 0.5, np.float32)
    mse = np.full(N_MSE, 1.0e36, np.float32)  # sum 1.024e39 > FLT_MAX = 3.4e38
    ce, om, flag, _ = _finalize(hip, rows, mse, 1.0, flag0=0.0)
    assert np.isposinf(om) and flag == 1.0 and ce == 0.5
    ce, om, flag, _ = _finalize(hip, rows, np.full(N_MSE, 3.0e38, np.float32), 1.0 / N_MSE, flag0=1.0)
    assert flag == 0.0 and _bit(om) == _bit(F32(3.0e38)), "the same sum scaled back into range is fine"


@pytest.mark.parametrize("with_flag", [False, True])
@pytest.mark.parametrize("with_step", [False, True])
@pytest.mark.parametrize("bad", [False, True])
def test_loss_finalize_nullable_flag_and_step(hip, with_flag, with_step, bad):
    """flag and step each NULL or given; the counter increments exactly when it is given, bad step or not, and carries
    from 2^32 - 1 into 2^32."""
    rows = np.arange(1, 258, dtype=np.float32)
    if bad:
        rows[100] = np.nan
    for step0 in (41, 2 ** 32 - 1):
        ce, _, flag, step = _finalize(hip, rows, with_flag=with_flag, with_step=with_step, flag0=0.0 if bad else 1.0,
                                      step0=step0)
        if with_flag:
            assert flag == (1.0 if bad else 0.0)
        if with_step:
            assert step == step0 + 1
        if not bad:
            assert ce == 129.0  # mean of 1..257


@pytest.mark.parametrize("n_rows", [1, 255, 256, 257, 1000])
def test_loss_finalize_plain_values(hip, n_rows):
    """fp64 sums, one rounding to fp32: within 1 fp32 ulp of the float64 result (half an ulp from the rounding; the
    order of the float64 additions moves the sum by a few 2^-53, which can flip that rounding at most one ulp)."""
    rng = np.random.default_rng(900 + n_rows)
    rows = (rng.random(n_rows) * 10.0 ** rng.uniform(-3, 1, n_rows)).astype(np.float32)
    mse = (rng.random(N_MSE) * 1e4).astype(np.float32)
    scale = 1.0 / (64 * 7105)
    ce, om, flag, step = _finalize(hip, rows, mse, scale, flag0=1.0)
    want_ce = _mean64(rows)
    want_mse = math.fsum(float(t) for t in mse) * scale
    assert flag == 0.0 and step == 42
    assert abs(float(ce) - want_ce) <= np.spacing(F32(want_ce)), (ce, want_ce)
    assert abs(float(om) - want_mse) <= np.spacing(F32(want_mse)), (om, want_mse)


# ============================================================================= softmax cross entropy, large logits
# Accuracy of the device expf / logf, measured on an MI355X with tools/exp/probe/libm_ulp_probe.hip (8192 arguments
# per range, against the host's double exp / log):
#   expf on [-87, 0]      0.7932 ulp        expf on [-104, -87] (subnormal results)   0.9983 ulp
#   expf below -104.5     exactly 0         logf on [1, 16]                           2.1715 ulp
# The device libm carries no written ulp contract and the grid is a sample, hence the factor 2 on top.
EXPF_ULP_MEASURED = 0.9983
LOGF_ULP_MEASURED = 2.1715
LIBM_MARGIN = 2.0


def _xent_rows(c, n):
    """Six kinds of row, cycled so that both blocks (rows 0..127, 128..129) meet several of them.  No logit is -inf:
    0 * (-inf) is NaN in the reference program's definition of the loss (labels * log_softmax) too, so a zero label on
    a -inf logit has no finite answer to hold the kernel to."""
    rng = np.random.default_rng(700 + c)
    z = np.zeros((n, c), np.float32)
    lab = np.zeros((n, c), np.float32)
    kind = np.arange(n) % 6
    for i in range(n):
        j0, j1 = i % c, (i + 1) % c
        if kind[i] in (0, 1):    # one confident logit; the label on it (loss ~ 0) or on a small one (loss ~ 1e4)
            z[i] = 0.1 * rng.standard_normal(c)
            z[i, j0] = 1e4
            lab[i, j0 if kind[i] == 0 else j1] = 1.0
        elif kind[i] == 2:       # everything far below zero: only differences count
            z[i] = -1e4
            lab[i, j1] = 1.0
        elif kind[i] == 3:       # label exactly 200 below the maximum: exp(-200) is 0 in fp32, the loss is 200 + lse
            z[i] = 95.0 + rng.standard_normal(c)
            z[i, j0], z[i, j1] = 100.0, -100.0
            lab[i, j1] = 1.0
        elif kind[i] == 4:       # all-zero label row: loss and gradient exactly 0
            z[i] = 5.0 * rng.standard_normal(c)
        else:                    # soft labels summing to 1
            z[i] = 50.0 * rng.standard_normal(c)
            lab[i] = rng.dirichlet(np.ones(c))
    return z, lab, kind


@pytest.mark.parametrize("c", [2, 15])
def test_softmax_xent_large_logits(hip, c):
    """Reference: float64 log-sum-exp on the same fp32 inputs.  n = 130 = one full block of 128 rows + 2, padded ld /
    ldl / lddl with poison in the padding.

    The kernel: t_j = z_j - zmax; se = sum_j expf(t_j); lse = logf(se); loss = -sum_j lab_j (t_j - lse);
    d_j = gscale (expf(t_j) / se * sum(lab) - lab_j).  With E, G the error of expf, logf in ulps (1 ulp <= 2 U relative),
    labels >= 0 of sum L <= 1, and every t_j - lse <= 0 (so the loss terms do not cancel):
      se:   c - 1 additions, expf (2 E U), and the rounding of t_j inside the exponential, sum_j s_j |t_j| U <= ln(c) U
            (entropy bound)                                         |d se| / se <= (c - 1 + 2 E + ln c) U
      lse:  that, plus logf on [0, ln c]:                           |d lse| <= (c - 1 + 2 E + ln c + 2 G ln c) U
      loss: per term the rounding of t_j, of t_j - lse and of the product (3 U of the term), c accumulations (c U of the
            loss), and L times d lse:                |d loss| <= (2 c + 2 + ln c + 2 E + 2 G ln c) U max(1, loss)
      d_j:  expf twice (numerator, se) 4 E, t_j in the numerator 0.37 (max of |t| e^t), in se ln c, se's c - 1 additions,
            sum(lab)'s c - 1, the reciprocal, two products, the difference, gscale: 5
                                                     |d d_j| <= (2 (c - 1) + ln c + 5.37 + 4 E) U |gscale| L
    E and G: measured on the device (tools/exp/probe/libm_ulp_probe.hip: expf on [-87, 0] and, subnormal results,
    [-104, -87]: 0.9983 ulp; logf on [1, 16]: 2.1715 ulp; 8192 arguments each), printed below, and doubled as the
    margin: E = 2.0, G = 4.3.  That gives 16.7 U for the loss and 16.0 U for dlogits at c = 2, 62.2 U and 44.1 U at
    c = 15."""
    e_ulp, g_ulp = LIBM_MARGIN * EXPF_ULP_MEASURED, LIBM_MARGIN * LOGF_ULP_MEASURED
    print(f"expf measured {EXPF_ULP_MEASURED} ulp, logf measured {LOGF_ULP_MEASURED} ulp; margin x{LIBM_MARGIN}")
    n, ld, ldl, lddl = 130, c + 3, c + 1, c + 2
    gscale = F32(1.0 / n)
    z, lab, kind = _xent_rows(c, n)
    zp = np.full((n, ld), 3e38, np.float32)        # a kernel that read the padding would see a huge maximum
    zp[:, :c] = z
    lp = np.full((n, ldl), 7.0, np.float32)
    lp[:, :c] = lab
    loss_t = hip.upload(np.full(n + 8, SENT, np.float32))
    d_t = hip.upload(np.full(n * lddl + 8, SENT, np.float32))
    hip.call("softmax_xent", Ref(hip.upload(zp)), ld, n, c, Ref(hip.upload(lp)), ldl, Ref(loss_t), Ref(d_t), lddl,
             float(gscale))
    loss, d = _host(loss_t), _host(d_t)
    assert np.array_equal(_bits(loss[n:]), _bits(np.full(8, SENT))) and np.array_equal(_bits(d[n * lddl:]), _bits(np.full(8, SENT)))
    loss, d = loss[:n], d[:n * lddl].reshape(n, lddl)
    assert np.array_equal(_bits(d[:, c:]), _bits(np.full((n, lddl - c), SENT))), "padding columns of dlogits"
    d = d[:, :c]

    z64, l64 = z.astype(np.float64), lab.astype(np.float64)
    t64 = z64 - z64.max(1, keepdims=True)
    se = np.exp(t64).sum(1, keepdims=True)
    want_loss = -(l64 * (t64 - np.log(se))).sum(1)
    lsum = l64.sum(1, keepdims=True)
    want_d = float(gscale) * (np.exp(t64) / se * lsum - l64)
    assert (lsum <= 1 + 1e-6).all()

    assert np.isfinite(loss).all() and np.isfinite(d).all()
    lnc = math.log(c)
    k_loss = 2 * c + 2 + lnc + 2 * e_ulp + 2 * g_ulp * lnc
    k_d = 2 * (c - 1) + lnc + 5.37 + 4 * e_ulp
    _report("loss", np.abs(loss - want_loss), k_loss * U * np.maximum(1.0, np.abs(want_loss)) * SLACK)
    err_d = np.abs(d - want_d)
    bound_d = np.broadcast_to(k_d * U * float(gscale) * lsum * SLACK, d.shape)
    assert (err_d[kind == 4] == 0).all() and (loss[kind == 4] == 0).all(), "all-zero label rows: loss and gradient 0"
    live = np.broadcast_to(lsum > 0, d.shape)
    _report("dlogits", err_d[live], bound_d[live])
    # what the rows are there for, in the reference itself
    assert (want_loss[kind == 0] < 1e-6).all() and (np.abs(want_loss[kind == 1] - 1e4) < 1.0).all()
    assert np.allclose(want_loss[kind == 2], lnc) and (want_loss[kind == 3] >= 200.0).all() and (want_loss[kind == 3] < 203.0).all()


# ================================================================================================ fill, rstd
@pytest.mark.parametrize("count", [0, 1, 1025, 524288 + 3])
def test_fill_f32(hip, count):
    """Base one element past a 16-byte boundary; 524288 + 3 takes a second grid sweep.  Bits compared as uint32 (-0.0 is
    not +0.0); NaN: any NaN.  Sentinels on both sides, and the range itself starts as sentinels."""
    for value in (0.0, -0.0, 7.5, np.nan):
        buf = hip.upload(np.full(1 + count + 8, SENT, np.float32))
        assert buf.data_ptr() % 16 == 0
        hip.call("fill_f32", Ref(buf, 1), count, float(value))
        got = _host(buf)
        assert _bits(got)[0] == _bit(SENT) and np.array_equal(_bits(got[1 + count:]), _bits(np.full(8, SENT)))
        body = got[1:1 + count]
        if np.isnan(value):
            assert np.isnan(body).all()
        else:
            assert np.array_equal(_bits(body), _bits(np.full(count, value, np.float32))), value


@pytest.mark.parametrize("c", [1, 63, 64, 65, 7105])
@pytest.mark.parametrize("eps", [1e-3, 1e-12])
def test_rstd_from_var(hip, c, eps):
    """rstd = fp32(1 / sqrt(fp64(var) + fp64(fp32(eps)))): the kernel works in fp64 and rounds once, so it is within
    1 fp32 ulp of the same expression in NumPy float64 (half an ulp from the rounding, the rest for a last-bit
    difference of the fp64 square root or division)."""
    rng = np.random.default_rng(c)
    var = np.resize(np.array([0.0, 1e-30, 1.0, 3e38], np.float32), c)
    var[4:] *= rng.random(max(0, c - 4)).astype(np.float32)
    out = hip.upload(np.full(c + 8, SENT, np.float32))
    hip.call("rstd_from_var", Ref(hip.upload(var)), c, float(eps), Ref(out))
    got = _host(out)
    assert np.array_equal(_bits(got[c:]), _bits(np.full(8, SENT))), "wrote past c"
    want = (1.0 / np.sqrt(var.astype(np.float64) + float(F32(eps)))).astype(np.float32)
    assert np.isfinite(got[:c]).all()
    assert (_ulps(got[:c], want) <= 1).all(), f"worst {_ulps(got[:c], want).max()} ulp"
