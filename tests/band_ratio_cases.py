"""TEST INFRASTRUCTURE: the inputs the band-ratio tests share (tests/test_band_ratio_emu.py on the NumPy twins,
tests/test_gpu_band_ratio.py on the device).  Everything is seeded and small: the shapes straddle a wavefront (63, 64,
65 rows), the 32-column histogram tile and the 64-lane band walk (1, 7, 65, 144 bands), and 4099 rows make more than
one row slice per column tile."""
import numpy as np

ROWS = (1, 63, 64, 65, 4099)
BANDS = (1, 7, 65, 144)
SHAPES = [(n, b) for n in ROWS for b in BANDS]
DATA_SETS = ("uniform", "ties90", "equal", "two_values", "zeros", "magnitudes")
RANK_COUNTS = (1, 6, 8)


def _name_code(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))


def ratio_case(n, bands, pad):
    """num, den [n, bands + pad] float32 (the first `bands` columns are the matrix: a row stride larger than the
    width), scale [bands].  Denominators hold exact zeros -- under a zero numerator (NaN) and a non-zero one (inf) --
    there are negative values, denormal numerators and denominators, and quotients that overflow and underflow."""
    rng = np.random.default_rng([n, bands, pad, 11])
    num = rng.standard_normal((n, bands + pad)).astype(np.float32)
    den = (rng.standard_normal((n, bands + pad)) * 0.7).astype(np.float32)
    pick = rng.random((n, bands + pad))
    den[pick < 0.02] = 0.0
    num[(pick < 0.004)] = 0.0                        # 0 / 0
    den[(pick > 0.02) & (pick < 0.03)] = -0.0
    num[(pick > 0.10) & (pick < 0.13)] = np.float32(1e-41)    # denormal numerator
    den[(pick > 0.20) & (pick < 0.23)] = np.float32(-3e-42)   # denormal denominator: large or infinite quotient
    num[(pick > 0.30) & (pick < 0.32)] *= np.float32(1e30)
    den[(pick > 0.40) & (pick < 0.42)] *= np.float32(1e30)
    if n > 8:  # most rows stay finite, so that both values of the mask occur at every shape
        clean = rng.random(n) < 0.6
        den[clean] = np.where(np.abs(den[clean]) < 0.05, np.float32(0.5), den[clean])
        num[clean] = np.clip(num[clean], -4, 4)
    scale = (rng.random(bands) * 3 + 0.1).astype(np.float32)
    scale[::5] *= -1
    return num, den, scale


def expected_ratio(num, den, scale, bands):
    """NumPy's own float32 expression: the reference of the ratio launch, bit for bit."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        r = num[:, :bands] / den[:, :bands]
        if scale is not None:
            r = r * scale
    assert r.dtype == np.float32
    return r, np.isfinite(r).all(axis=1)


def column_data(kind, n, bands, rng):
    if kind == "uniform":
        x = rng.random((n, bands)) * 4 - 1
    elif kind == "ties90":
        x = np.where(rng.random((n, bands)) < 0.9, 1.25, rng.standard_normal((n, bands)))
    elif kind == "equal":
        x = np.full((n, bands), -0.75)
    elif kind == "two_values":
        x = np.where(rng.random((n, bands)) < 0.5, 2.0, -3.0)
    elif kind == "zeros":
        x = rng.choice(np.float32([0.0, -0.0, 1e-45, -1e-45, 1.0]), size=(n, bands), p=[0.4, 0.4, 0.08, 0.08, 0.04])
    elif kind == "magnitudes":
        x = np.sign(rng.standard_normal((n, bands))) * 10.0 ** rng.uniform(-30, 30, (n, bands))
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


def kept_counts(n):
    return sorted({m for m in (1, 2, n - 1, n) if 1 <= m <= n})


def ranks_for(m, count):
    """`count` ranks in [0, m): the ends, the middle, a repeat, unsorted"""
    if count == 1:
        return [m // 2]
    return [m // 2, 0, m - 1, m // 2, m // 3, (2 * m) // 3, m - 1, 0][:count]


def select_case(kind, n, bands, m, pad):
    """x [n, bands + pad] float32 and row_ok [n] uint8 with m rows kept; the rows masked out are NaN and infinities,
    which the launch must never read as values."""
    rng = np.random.default_rng([n, bands, m, pad, _name_code(kind)])
    x = np.full((n, bands + pad), np.float32(np.nan))
    x[:, :bands] = column_data(kind, n, bands, rng)
    keep = np.zeros(n, bool)
    keep[rng.permutation(n)[:m]] = True
    poison = np.float32([np.nan, np.inf, -np.inf])
    x[~keep] = poison[rng.integers(0, 3, ((~keep).sum(), bands + pad))]
    return x, keep.astype(np.uint8)


def expected_select(x, row_ok, bands, ranks):
    return np.sort(x[row_ok != 0][:, :bands], axis=0)[np.asarray(ranks)]


def stats_cases():
    """(name, num, den, scale) for band_ratio_stats against numpy.percentile: ties, rows masked by a zero denominator,
    one row, an even and an odd count, and a few thousand rows."""
    out = []
    for n, bands, ties in ((1, 5, False), (2, 3, False), (7, 16, True), (64, 33, False), (301, 12, True),
                           (4099, 20, False), (9973, 4, True)):
        rng = np.random.default_rng([n, bands, 5])
        den = (rng.random((n, bands)) + 0.25).astype(np.float32)
        num = (den * (0.4 + 0.2 * rng.standard_normal((n, bands)))).astype(np.float32)
        if ties:
            num = np.where(rng.random((n, bands)) < 0.7, den * np.float32(0.5), num).astype(np.float32)
        if n > 4:
            den[rng.random(n) < 0.1, 0] = 0.0  # masked rows: inf or NaN in band 0
        scale = None if n % 2 == 0 else (rng.random(bands) + 0.5).astype(np.float32)
        out.append((f"n{n}_b{bands}", num, den, scale))
    return out
