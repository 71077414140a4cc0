"""TEST INFRASTRUCTURE: numpy twin of the pixel-pairing entry points (include/hypel.h: hypel_mask_dilate_l1_u8,
hypel_pair_masks_u8, hypel_mask_compact_points_i32, hypel_points_expand_i32), attached to tests/emu_backend.EmuBackend
on import.  An executable specification of each launch's contract written from the header; the dilation is the
definition itself -- a brute-force L1 distance to every set pixel -- not a restatement of the kernel's two passes."""
import numpy as np

from hypelcnn_amd.backend import COMPACT_TILE
from tests.emu_backend import EmuBackend
from tests.emu_scene import _typed


def dilate_l1(smap, radius):
    """out[y, x] = 1 where a pixel with smap != 0 lies within L1 distance `radius`; outside the raster counts as 0"""
    on = np.asarray(smap) != 0
    h, w = on.shape
    out = np.zeros((h, w), bool)
    # every offset (dy, dx) of the L1 ball, tried one by one: out[y, x] |= on[y + dy, x + dx] where that is inside
    for dy in range(-min(radius, h - 1), min(radius, h - 1) + 1):
        reach = min(radius - abs(dy), w - 1)
        for dx in range(-reach, reach + 1):
            out[max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)] |= \
                on[max(0, dy):h - max(0, -dy), max(0, dx):w - max(0, -dx)]
    return out.astype(np.uint8)


def _k_mask_dilate_l1_u8(self, map_, h, w, radius, out, ws):
    assert radius >= 1 and ws is not None and ws.t.numel() - ws.off >= h * w
    _typed(out, np.uint8, h * w)[:] = dilate_l1(_typed(map_, np.uint8, h * w).reshape(h, w), radius).reshape(-1)


def _k_pair_masks_u8(self, map_, reach, margin, n, shadow, lit):
    assert (reach is None) == (margin is None)
    m = _typed(map_, np.uint8, n)
    sel = m != 1
    if reach is not None:
        sel = sel & (_typed(reach, np.uint8, n) != 0) & (_typed(margin, np.uint8, n) == 0)
    _typed(shadow, np.uint8, n)[:] = m == 1
    _typed(lit, np.uint8, n)[:] = sel


def _k_mask_compact_points_i32(self, mask, h, w, points, capacity, count, ws):
    assert h * w < 2 ** 31 and ws.t.numel() - ws.off >= (h * w + COMPACT_TILE - 1) // COMPACT_TILE
    ys, xs = np.nonzero(_typed(mask, np.uint8, h * w).reshape(h, w))  # row-major scan order
    keep = min(int(capacity), ys.size)
    _typed(points, np.int32, 2 * keep).reshape(keep, 2)[:] = np.stack([xs, ys], axis=1)[:keep]
    _typed(count, np.int32, 1)[0] = ys.size


def _k_points_expand_i32(self, points, n, repeat, remainder, out):
    assert n > 0 and repeat >= 0 and 0 <= remainder <= n and n * repeat + remainder > 0
    p = _typed(points, np.int32, 2 * n).reshape(n, 2)
    total = n * repeat + remainder
    _typed(out, np.int32, 2 * total).reshape(total, 2)[:] = np.vstack([np.repeat(p, repeat, axis=0), p[0:remainder]])


for _name, _fn in list(globals().items()):
    if _name.startswith("_k_"):
        setattr(EmuBackend, _name[1:], _fn)
