"""TEST INFRASTRUCTURE: numpy twin of the template-matching entry points (include/hypel.h: hypel_match_ccorr_f32,
hypel_match_window_energy_f64, hypel_match_best_f32, hypel_match_render_u8), attached to tests/emu_backend.EmuBackend on
import.  An executable specification of each launch's contract written from the header, by other means than the
reference of tests/match_cases.py: the replication is an index look-up, the numerator is accumulated tap by tap over
shifted slices of the image (float64, rounded to float32 once -- inside the launch's bound, and exact for the integer
cases), the window energies come from a summed-area table."""
import numpy as np

from hypelcnn_amd.backend import MATCH_MAX_SPLITS
from tests.emu_backend import EmuBackend
from tests.emu_scene import _typed

LIMIT = 2 ** 31


def _band(ref, h, w, sy, sx, scale):
    """the enlarged band [h * scale, w * scale] as float64"""
    assert h > 0 and w > 0 and sy >= 0 and sx >= 0 and scale >= 1 and h * scale * w * scale < LIMIT
    flat = _typed(ref, np.float32)
    assert (h - 1) * sy + (w - 1) * sx < flat.size, "the strided raster reaches past its buffer"
    ys, xs = np.arange(h * scale) // scale, np.arange(w * scale) // scale
    return flat[ys[:, None] * sy + xs[None, :] * sx].astype(np.float64)


def _k_match_ccorr_f32(self, image, h, w, sy, sx, scale, tmpl, ht, wt, tsy, tsx, tscale, num, ws, splits):
    big, tpl = _band(image, h, w, sy, sx, scale), _band(tmpl, ht, wt, tsy, tsx, tscale)
    hout, wout = big.shape[0] - tpl.shape[0] + 1, big.shape[1] - tpl.shape[1] + 1
    assert hout >= 1 and wout >= 1 and 1 <= splits <= MATCH_MAX_SPLITS and hout * wout * splits < LIMIT
    if splits > 1:
        assert ws is not None and _typed(ws, np.float32).size >= splits * hout * wout
    acc = np.zeros((hout, wout))
    for i in range(tpl.shape[0]):
        for j in range(tpl.shape[1]):
            acc += tpl[i, j] * big[i:i + hout, j:j + wout]
    _typed(num, np.float32, hout * wout)[:] = acc.astype(np.float32).reshape(-1)


def _k_match_window_energy_f64(self, src, h, w, sy, sx, scale, win_h, win_w, energy, ws):
    big = _band(src, h, w, sy, sx, scale)
    H, W = big.shape
    assert 1 <= win_h <= H and 1 <= win_w <= W
    hout, wout = H - win_h + 1, W - win_w + 1
    assert _typed(ws, np.float64).size >= h * wout
    table = np.zeros((H + 1, W + 1))
    table[1:, 1:] = (big * big).cumsum(axis=0).cumsum(axis=1)
    sums = table[win_h:, win_w:] - table[:hout, win_w:] - table[win_h:, :wout] + table[:hout, :wout]
    _typed(energy, np.float64, hout * wout)[:] = np.maximum(sums, 0.0).reshape(-1)


def _k_match_best_f32(self, num, energy, e_t, hout, wout, score_map, result):
    n = hout * wout
    assert 0 < n < LIMIT
    d = _typed(energy, np.float64, n) * _typed(e_t, np.float64, 1)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, _typed(num, np.float32, n).astype(np.float64) / np.sqrt(d)).astype(np.float32)
    if score_map is not None:
        _typed(score_map, np.float32, n)[:] = r
    best = int(np.argmax(r))  # the first of equal maxima
    record = _typed(result, np.uint8, 16)
    record[:] = 0
    record[0:4] = np.array([r[best]], np.float32).view(np.uint8)
    record[8:16] = np.array([best], np.int64).view(np.uint8)


def _k_match_render_u8(self, src, h, w, sy, sx, scale, max_, out):
    big = _band(src, h, w, sy, sx, scale).astype(np.float32)
    top = _typed(max_, np.float32, 1)[0]
    if top > 0:
        grey = big / top * np.float32(255)
        assert grey.dtype == np.float32
        levels = np.clip(grey, 0, 255).astype(np.uint8)  # truncation
    else:
        levels = np.zeros(big.shape, np.uint8)
    _typed(out, np.uint8, levels.size)[:] = levels.reshape(-1)


for _name, _fn in list(globals().items()):
    if _name.startswith("_k_"):
        setattr(EmuBackend, _name[1:], _fn)
