"""TEST INFRASTRUCTURE: inputs, float64 references and derived error bounds for the band-PCA launches and BandPCA, shared
by tests/test_pca_emu.py (NumPy twin) and tests/test_gpu_pca.py (device).

Every bound here is derived, not tuned (u = 2^-24, the float32 unit roundoff):
 * sums       |sum - sum64| <= n * 2^-53 * sum|x|: n double additions of exact values, in any order.
 * scatter    |S_ij - S64_ij| <= (CHUNK + 4) * u * sqrt(S64_ii * S64_jj), S64 the float64 scatter about the SAME float32
              mean: the centring rounds each factor once (2 u |d_i d_j| per product, to first order), one float32
              accumulator adds at most CHUNK products (CHUNK u sum|d_i d_j|), and sum|d_i d_j| <= sqrt(S_ii S_jj)
              (Cauchy-Schwarz); the double additions of the chunk partials and the second-order terms fit in the
              remaining 2 u.
 * projection |out_rj - out64_rj| <= (c + 2) * u * sum_b |d_b| |W_bj| with d = x - mean in float64: one rounding of the
              centring and c of the fmaf chain per term, second-order terms in the remaining u.
 * BandPCA    the covariance is S / (n - 1) minus an exactly known rank-one term, so |dC_ij| <= (CHUNK + 4) u
              sqrt(C'_ii C'_jj) with C' = S64 / (n - 1), and ||dC||_2 <= ||dC||_F <= (CHUNK + 4) u trace(C').  Weyl:
              every eigenvalue moves by at most ||dC||_2.  Davis-Kahan (sin theta form, one-dimensional invariant
              subspace): sin(angle) <= 2 ||dC||_2 / gap, gap the distance to the nearest other eigenvalue.  The float64
              eigh of the reference itself is trusted to c * 2^-52 * ||C||, added to both."""
import numpy as np

from hypelcnn_amd.backend import PCA_CHUNK, Ref
from hypelcnn_amd.classic.decomposition import band_sums_ws_doubles, scatter_ws_doubles

U24 = 2.0 ** -24
BANDS = (1, 3, 15, 16, 17, 33, 64, 144, 145, 360, 512)
PIXELS = (2, 63, 64, 65, PCA_CHUNK - 1, PCA_CHUNK, PCA_CHUNK + 1)
SENTINEL = 0x5A


def hard_pixels(n, c, seed=0):
    """float32 [n, c] like the raw uint16 scenes: band means of 2000 to 12000, standard deviations from 30 down to 0.007
    (geometrically), and -- from 3 bands on -- one constant band (index c // 2)."""
    rng = np.random.default_rng([seed, n, c])
    mean = rng.uniform(2000.0, 12000.0, c)
    std = 30.0 * (0.007 / 30.0) ** (np.arange(c) / max(1, c - 1))
    x = (mean[None, :] + std[None, :] * rng.standard_normal((n, c))).astype(np.float32)
    if c >= 3:
        x[:, c // 2] = np.float32(mean[c // 2])
    return x


def factor(n):
    """n = h * w with h the largest divisor of n that is at most sqrt(n)"""
    h = int(np.sqrt(n))
    while n % h:
        h -= 1
    return h, n // h


def layouts(x):
    """The same pixels as (name, float32 buffer, origin in floats, h, w, stride_y, stride_x): a plain row matrix, the
    interior of a padded scene [h + 4][w + 4][C] (neighbourhood 2, C odd >= c) that starts one float into its buffer --
    the origin is 4-byte aligned only and stride_y != w * stride_x -- and the interior of the same scene stored
    [w + 4][h + 4][C]: stride_y < stride_x, consecutive pixels of a row lie a whole stored line apart."""
    n, c = x.shape
    yield "plain", x.reshape(-1).copy(), 0, 1, n, n * c, c
    h, w = factor(n)
    cs = c if c % 2 else c + 1
    scene = np.full((h + 4, w + 4, cs), np.float32(np.nan))  # what lies outside the view is never read
    scene[2:2 + h, 2:2 + w, :c] = x.reshape(h, w, c)
    buf = np.concatenate([np.full(1, np.nan, np.float32), scene.reshape(-1)])
    yield "padded", buf, 1 + 2 * (w + 4 + 1) * cs, h, w, (w + 4) * cs, cs
    scene = np.full((w + 4, h + 4, cs), np.float32(np.nan))
    scene[2:2 + w, 2:2 + h, :c] = x.reshape(h, w, c).transpose(1, 0, 2)
    buf = np.concatenate([np.full(1, np.nan, np.float32), scene.reshape(-1)])
    yield "transposed", buf, 1 + 2 * (h + 4 + 1) * cs, h, w, cs, (h + 4) * cs


def guarded(be, count, dtype):
    """a device byte buffer of `count` items of dtype between two 64-byte guards of SENTINEL, as (tensor of the items, check)"""
    import torch
    item = np.dtype(dtype).itemsize
    raw = be.upload(np.full(128 + count * item, SENTINEL, np.uint8))
    body = raw[64:64 + count * item].view({4: torch.float32, 8: torch.float64}[item])

    def intact():
        host = raw.cpu().numpy()
        return bool((host[:64] == SENTINEL).all() and (host[64 + count * item:] == SENTINEL).all())
    return body, intact


def run_fit_launches(be, buf, origin, h, w, c, stride_y, stride_x):
    """The two fit launches on one layout -> (sums float64 [c], mean32, scatter float64 [c, c]); the outputs lie between
    sentinel bytes that must survive, the workspaces are exactly as long as the header asks."""
    n = h * w
    x_d = be.upload(buf)
    sums, sums_ok = guarded(be, c, np.float64)
    ws, ws_ok = guarded(be, band_sums_ws_doubles(n, c), np.float64)
    be.call("pca_band_sums_f64", Ref(x_d, origin), h, w, c, stride_y, stride_x, Ref(sums), Ref(ws), ws.numel())
    sums_h = sums.cpu().numpy().copy()
    assert sums_ok() and ws_ok()
    mean32 = (sums_h / n).astype(np.float32)
    scatter, scatter_ok = guarded(be, c * c, np.float64)
    ws, ws_ok = guarded(be, scatter_ws_doubles(n, c), np.float64)
    be.call("pca_scatter_f64", Ref(x_d, origin), h, w, c, stride_y, stride_x, Ref(be.upload(mean32)), Ref(scatter), Ref(ws),
            ws.numel())
    scatter_h = scatter.cpu().numpy().copy().reshape(c, c)
    assert scatter_ok() and ws_ok()
    return sums_h, mean32, scatter_h


def check_fit_launches(x, sums, mean32, scatter):
    """-> (largest sums error / its bound, largest scatter error / its bound), after asserting both bounds"""
    n, c = x.shape
    x64 = x.astype(np.float64)
    sums_bound = n * 2.0 ** -53 * np.abs(x64).sum(0)
    sums_err = np.abs(sums - x64.sum(0))
    assert (sums_err <= sums_bound).all(), (sums_err / sums_bound).max()
    d = x64 - mean32.astype(np.float64)[None, :]
    s64 = d.T @ d
    diag = np.sqrt(np.diag(s64))
    bound = (PCA_CHUNK + 4) * U24 * np.outer(diag, diag)
    err = np.abs(scatter - s64)
    assert (err <= bound).all(), float((err / np.where(bound > 0, bound, 1)).max())
    assert np.array_equal(scatter, scatter.T)
    if c >= 3:  # the constant band: a row and a column of exact zeros
        assert not scatter[c // 2].any() and not scatter[:, c // 2].any()
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(sums_err / sums_bound)), float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))


def projection_bound(x, c, mean32, weights32):
    """(float64 reference [n, k], elementwise bound [n, k]) of hypel_pca_project_f32 on the first c columns of x"""
    d = x[:, :c].astype(np.float64) - mean32.astype(np.float64)[None, :]
    w = weights32.astype(np.float64)
    return d @ w, (c + 2) * U24 * (np.abs(d) @ np.abs(w))


def spectrum_pixels(n, c, ratio=4.0, seed=0, top=900.0):
    """float32 [n, c] whose covariance has the geometric eigenvalue spectrum top, top / ratio, ... in a random basis,
    under band means of 2000 to 12000: every component has a wide gap."""
    rng = np.random.default_rng([seed, n, c, 77])
    basis, _ = np.linalg.qr(rng.standard_normal((c, c)))
    scale = np.sqrt(top * ratio ** -np.arange(c, dtype=np.float64))
    return (rng.uniform(2000.0, 12000.0, c)[None, :] + (rng.standard_normal((n, c)) * scale[None, :]) @ basis.T).astype(np.float32)


def covariance_bound(x, mean, top):
    """||dC||_2 of the module docstring for a fit of x (float32 [n, c]) whose float64 mean is `mean`; top: the largest
    eigenvalue of the reference"""
    n, c = x.shape
    d = x.astype(np.float64) - mean.astype(np.float32).astype(np.float64)[None, :]
    return (PCA_CHUNK + 4) * U24 * np.trace(d.T @ d) / (n - 1) + c * 2.0 ** -52 * top


def check_against_eigh(pca, x):
    """BandPCA fitted on x (float32 [n, c]) against numpy.linalg.eigh of the float64 covariance of the same input, within
    the bounds of the module docstring.  -> (largest eigenvalue error / bound, largest sine / bound)"""
    n, c = x.shape
    x64 = x.astype(np.float64)
    cov = np.cov(x64.T).reshape(c, c)
    values, vectors = np.linalg.eigh(cov)
    values, vectors = values[::-1], vectors[:, ::-1].T
    d_c = covariance_bound(x, pca.mean_, values[0])
    k = pca.n_components_
    # (the sums bound over n, once for the launch, once for NumPy's own sum, once for the two divisions)
    assert (np.abs(pca.mean_ - x64.mean(0)) <= 3 * n * 2.0 ** -53 * np.abs(x64).mean(0)).all()
    value_err = np.abs(pca.explained_variance_ - np.clip(values[:k], 0, None))
    assert (value_err <= d_c).all(), (value_err / d_c).max()
    assert np.allclose(pca.explained_variance_ratio_, pca.explained_variance_ / np.clip(values, 0, None).sum(), rtol=1e-6)
    worst = 0.0
    for i in range(k):
        others = np.delete(values, i)
        gap = np.abs(others - values[i]).min()
        cosine = abs(float(pca.components_[i] @ vectors[i]))
        sine = np.sqrt(max(0.0, 1.0 - min(1.0, cosine) ** 2))
        assert sine <= 2 * d_c / gap + 1e-7, (i, sine, 2 * d_c / gap)  # (1e-7: sqrt(1 - cos^2) of a float64 cosine)
        worst = max(worst, sine / (2 * d_c / gap + 1e-7))
        lead = int(np.argmax(np.abs(pca.components_[i])))
        assert pca.components_[i][lead] > 0
    assert abs(np.linalg.norm(pca.components_, axis=1) - 1).max() < 1e-12
    return float((value_err / d_c).max()), worst
