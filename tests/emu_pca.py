"""TEST INFRASTRUCTURE: NumPy twins of the band-PCA entry points (include/hypel.h, hypel_pca_*), attached to
tests/emu_backend.EmuBackend on import.  Written from the header.  Every launch is appended to the backend's `launch_log`.

What the twins promise: the argument checks of the entry points (an assertion where the library answers "invalid
argument"), the value each output has in the header, and results that do not depend on how the view lies in memory --
a view is gathered into a dense [pixels][bands] matrix first.  They do NOT promise the kernels' bits: the sums and the
scatter are float64 NumPy reductions in NumPy's order (the scatter of float32-centred values, chunk by chunk), and the
projection's fmaf chain is imitated as float32(float64(acc) + float64(d) * float64(w)) -- the product is exact in
float64, but the sum is rounded twice where fmaf rounds once, so a last bit can differ."""
import numpy as np

from hypelcnn_amd.backend import PCA_CHUNK, PCA_MAX_BANDS
from hypelcnn_amd.classic.decomposition import band_sums_ws_doubles, scatter_ws_doubles
from tests.emu_backend import EmuBackend, _arr

LIMIT = 1 << 40


def _pixels(x, h, w, c, stride_y, stride_x, tail=0):
    """the view as a dense float32 [h * w][c + tail] copy"""
    assert x is not None and 1 <= h <= LIMIT and 1 <= w <= LIMIT and h * w <= LIMIT and 1 <= c <= PCA_MAX_BANDS
    assert c + tail <= stride_y <= LIMIT and c + tail <= stride_x <= LIMIT
    a = _arr(x)
    assert (h - 1) * stride_y + (w - 1) * stride_x + c + tail <= a.size, "the view leaves its buffer"
    view = np.lib.stride_tricks.as_strided(a, shape=(h, w, c + tail), strides=(stride_y * 4, stride_x * 4, 4))
    return np.ascontiguousarray(view).reshape(h * w, c + tail)


def _k_pca_band_sums_f64(self, x, h, w, c, stride_y, stride_x, sums, ws, ws_doubles):
    self.launch_log.append("pca_band_sums_f64")
    px = _pixels(x, h, w, c, stride_y, stride_x)
    assert sums is not None and ws is not None and ws_doubles >= band_sums_ws_doubles(h * w, c)
    assert _arr(ws, np.float64).size >= ws_doubles
    _arr(sums, np.float64)[:c] = px.astype(np.float64).sum(0)


def _k_pca_scatter_f64(self, x, h, w, c, stride_y, stride_x, mean, scatter, ws, ws_doubles):
    self.launch_log.append("pca_scatter_f64")
    px = _pixels(x, h, w, c, stride_y, stride_x)
    assert mean is not None and scatter is not None and ws is not None and ws_doubles >= scatter_ws_doubles(h * w, c)
    assert _arr(ws, np.float64).size >= ws_doubles
    d = px - _arr(mean)[:c][None, :]  # float32: centred at load
    total = np.zeros((c, c), np.float64)
    for p0 in range(0, h * w, PCA_CHUNK):
        part = d[p0:p0 + PCA_CHUNK].astype(np.float64)
        total += part.T @ part
    total = np.triu(total) + np.triu(total, 1).T  # one half serves both
    _arr(scatter, np.float64)[:c * c] = total.reshape(-1)


def project_rows(px, c, mean, weights):
    """[n][>= c] float32 -> [n][k]: one chain over the bands per output, the same for every row"""
    d = (px[:, :c] - mean[None, :]).astype(np.float64)
    acc = np.zeros((px.shape[0], weights.shape[1]), np.float32)
    w64 = weights.astype(np.float64)
    for b in range(c):
        acc = (acc.astype(np.float64) + d[:, b:b + 1] * w64[b][None, :]).astype(np.float32)
    return acc


def _k_pca_project_f32(self, x, h, w, c, stride_y, stride_x, pass_, mean, weights, k, out, ldo):
    self.launch_log.append("pca_project_f32")
    assert 0 <= pass_ <= PCA_MAX_BANDS
    px = _pixels(x, h, w, c, stride_y, stride_x, pass_)
    assert mean is not None and weights is not None and out is not None and 1 <= k <= c and k + pass_ <= ldo <= LIMIT
    n = h * w
    o = _arr(out)
    assert (n - 1) * ldo + k + pass_ <= o.size, "the output leaves its buffer"
    assert not np.shares_memory(_arr(x)[:(h - 1) * stride_y + (w - 1) * stride_x + c + pass_], o[:(n - 1) * ldo + k + pass_])
    rows = np.lib.stride_tricks.as_strided(o, shape=(n, k + pass_), strides=(ldo * 4, 4))
    rows[:, :k] = project_rows(px, c, _arr(mean)[:c].copy(), _arr(weights)[:c * k].reshape(c, k).copy())
    rows[:, k:] = px[:, c:]


EmuBackend.k_pca_band_sums_f64 = _k_pca_band_sums_f64
EmuBackend.k_pca_scatter_f64 = _k_pca_scatter_f64
EmuBackend.k_pca_project_f32 = _k_pca_project_f32
