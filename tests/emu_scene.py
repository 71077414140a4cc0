"""TEST INFRASTRUCTURE: numpy twin of the scene-preparation entry points (include/hypel.h, hypel_scene_*), attached to
tests/emu_backend.EmuBackend on import.  An executable specification of each launch's contract written from the header:
buffers have the device's dtypes and layouts, the arithmetic is NumPy's own."""
import numpy as np

from hypelcnn_amd.backend import OUT_DTYPES
from tests.emu_backend import EmuBackend

DTYPE_OF = {code: dt for dt, code in OUT_DTYPES.items()}


def _typed(ref, dtype, count=None):
    """view of the (byte or typed) tensor behind a Ref from its offset on, as `dtype`"""
    if ref is None:
        return None
    raw = ref.t.numpy().reshape(-1)
    raw = raw.view(np.uint8)[ref.off * raw.dtype.itemsize:]
    item = np.dtype(dtype).itemsize
    n = raw.size // item if count is None else count
    return raw[: n * item].view(dtype)


def _source(ref, dtype, h, w, bands, sy, sx, sb):
    flat = _typed(ref, dtype)
    item = flat.dtype.itemsize
    span = (h - 1) * sy + (w - 1) * sx + (bands - 1) * sb + 1
    assert span <= flat.size, "the strided raster reaches past its buffer"
    return np.lib.stride_tricks.as_strided(flat, shape=(h, w, bands), strides=(sy * item, sx * item, sb * item))


def _clip_sub(v, dtype, bands, clip, sub):
    if clip is not None:
        v = np.minimum(v, _typed(clip, dtype, bands))
    if sub is not None:
        v = (v - _typed(sub, dtype, bands)).astype(dtype)  # the source dtype's own subtraction (integers wrap)
    return v


def _k_scene_extrema(self, src, dtype, h, w, bands, sy, sx, sb, clip, sub, out_min, out_max, ws, ws_slices):
    dt = DTYPE_OF[dtype]
    assert ws is not None and ws_slices > 0
    v = _clip_sub(_source(src, dt, h, w, bands, sy, sx, sb), dt, bands, clip, sub)
    _typed(out_min, dt, bands)[:] = v.min(axis=(0, 1))
    _typed(out_max, dt, bands)[:] = v.max(axis=(0, 1))


def _k_scene_rank_select_u16(self, src, h, w, bands, sy, sx, sb, rank_lo, rank_hi, out_lo, out_hi, ws):
    assert 0 <= rank_lo <= rank_hi < h * w and ws is not None
    v = np.sort(_source(src, np.uint16, h, w, bands, sy, sx, sb).reshape(h * w, bands), axis=0)
    _typed(out_lo, np.uint16, bands)[:] = v[rank_lo]
    _typed(out_hi, np.uint16, bands)[:] = v[rank_hi]


def _k_scene_prepare_f32(self, src, dtype, h, w, bands, sy, sx, sb, pad, clip, lo, scale, out):
    dt = DTYPE_OF[dtype]
    v = _clip_sub(_source(src, dt, h, w, bands, sy, sx, sb), dt, bands, clip, lo)
    v = np.pad(v, ((pad, pad), (pad, pad), (0, 0)), mode="symmetric").astype(np.float32)
    if scale is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            v = v / _typed(scale, np.float32, bands)
    _typed(out, np.float32, v.size)[:] = v.reshape(-1)


def _k_scene_masked_sums(self, scene, map_, hp, wp, bands, sums, counts, ws, ws_slices):
    assert ws is not None and ws_slices > 0
    s = _typed(scene, np.float32, hp * wp * bands).reshape(hp * wp, bands).astype(np.float64)
    on = _typed(map_, np.uint8, hp * wp) != 0
    out = _typed(sums, np.float64, 2 * bands).reshape(2, bands)
    out[0] = s[on].sum(axis=0)
    out[1] = s[~on].sum(axis=0)
    _typed(counts, np.int64, 2)[:] = [int(on.sum()), int((~on).sum())]


for _name, _fn in list(globals().items()):
    if _name.startswith("_k_scene_"):
        setattr(EmuBackend, _name[1:], _fn)
