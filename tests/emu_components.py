"""TEST INFRASTRUCTURE: numpy twin of the shadow-region entry points (include/hypel.h: hypel_components_label_u8,
hypel_components_compact_i32, hypel_components_votes_i32, hypel_components_relabel_u8, hypel_shadow_correct_f32),
attached to tests/emu_backend.EmuBackend on import.  An executable specification of each launch's contract written from
the header.  The labelling is neither the kernel's union-find nor the flood fill of tests/component_cases.py: every
pixel repeatedly takes the smallest label among itself and its 8 neighbours, hands it to the pixel its own label names,
and jumps to that pixel's label, until nothing moves -- whole-array NumPy steps, so the big random mask stays cheap."""
import numpy as np

from hypelcnn_amd.backend import COMPACT_TILE, COMPONENTS_MAX_CLASSES, COMPONENTS_OK
from tests.emu_backend import EmuBackend
from tests.emu_scene import DTYPE_OF, _source, _typed

OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` where that is outside"""
    h, w = a.shape
    out = np.full_like(a, fill)
    out[max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)] = a[max(0, dy):h - max(0, -dy), max(0, dx):w - max(0, -dx)]
    return out


def label_roots(mask):
    """root[y, x] = row-major index of the first pixel of the 8-connected component of (y, x), -1 outside the mask"""
    on = np.asarray(mask) != 0
    h, w = on.shape
    big = h * w
    lab = np.where(on, np.arange(h * w, dtype=np.int64).reshape(h, w), big)
    inside = np.flatnonzero(on)
    while inside.size:
        low = lab.copy()
        for dy, dx in OFFSETS:
            np.minimum(low, _shift(lab, dy, dx, big), out=low)
        flat = lab.reshape(-1).copy()
        np.minimum.at(flat, flat[inside], low.reshape(-1)[inside])  # the label's own pixel learns of the smaller one
        flat[inside] = np.minimum(flat[inside], low.reshape(-1)[inside])
        while True:  # jump: a label is a pixel of the same component, whose label is no larger
            nxt = flat.copy()
            nxt[inside] = flat[flat[inside]]
            if np.array_equal(nxt, flat):
                break
            flat = nxt
        if np.array_equal(flat, lab.reshape(-1)):
            break
        lab = flat.reshape(h, w)
    return np.where(on, lab, -1).astype(np.int32)


def _k_components_label_u8(self, mask, h, w, root, ws, status):
    assert 0 < h * w < 2 ** 31 and ws.t.numel() - ws.off >= h * w
    _typed(root, np.int32, h * w)[:] = label_roots(_typed(mask, np.uint8, h * w).reshape(h, w)).reshape(-1)
    _typed(status, np.int32, 1)[0] = COMPONENTS_OK


def _k_components_compact_i32(self, root, h, w, comp, n_components, ws):
    assert 0 < h * w < 2 ** 31 and ws.t.numel() - ws.off >= (h * w + COMPACT_TILE - 1) // COMPACT_TILE
    r = _typed(root, np.int32, h * w)
    is_root = r == np.arange(h * w)
    rank = np.cumsum(is_root) - 1  # of a root: the roots before it in row-major order
    _typed(comp, np.int32, h * w)[:] = np.where(r >= 0, rank[np.maximum(r, 0)], -1)
    _typed(n_components, np.int32, 1)[0] = int(is_root.sum())


def _k_components_votes_i32(self, targets, comp, h, w, n_components, n_classes, exclude, votes, size, winner):
    assert 1 <= n_classes <= COMPONENTS_MAX_CLASSES and 0 <= n_components <= h * w
    if n_components == 0:
        return
    t = _typed(targets, np.uint8, h * w).reshape(h, w).astype(np.int64)
    c = _typed(comp, np.int32, h * w).reshape(h, w).astype(np.int64)
    v = np.zeros((n_components, n_classes), np.int64)
    allowed = np.array([k < n_classes and not (int(exclude) >> k) & 1 for k in range(256)])
    for dy, dx in OFFSETS:
        tq, cq = _shift(t, dy, dx, 255), _shift(c, dy, dx, 0)  # outside the image: comp 0 -- "inside the mask", no vote
        says = (c >= 0) & (cq < 0) & allowed[tq]
        np.add.at(v, (c[says], tq[says]), 1)
    _typed(votes, np.int32, n_components * n_classes)[:] = v.reshape(-1)
    _typed(size, np.int32, n_components)[:] = np.bincount(c[c >= 0], minlength=n_components)
    best = v.argmax(axis=1)  # the first of equal maxima: the smallest class
    _typed(winner, np.uint8, n_components)[:] = np.where(v.max(axis=1) > 0, best, 255)


def _k_components_relabel_u8(self, targets, comp, winner, h, w, plus_one, out):
    t = _typed(targets, np.uint8, h * w)
    c = _typed(comp, np.int32, h * w)
    res = t.copy()
    if (c >= 0).any():
        win = _typed(winner, np.uint8, int(c.max()) + 1)[np.maximum(c, 0)]
        paint = (c >= 0) & (win != 255)
        res[paint] = win[paint]
    if plus_one:
        res[res != 255] += 1
    _typed(out, np.uint8, h * w)[:] = res


def _k_shadow_correct_f32(self, src, dtype, h, w, bands, sy, sx, sb, map_, r_minus_1, out):
    c = _source(src, DTYPE_OF[dtype], h, w, bands, sy, sx, sb).astype(np.float32)
    m = (_typed(map_, np.uint8, h * w).reshape(h, w, 1) != 0).astype(np.float32)
    coef = m * _typed(r_minus_1, np.float32, bands)
    assert coef.dtype == np.float32
    _typed(out, np.float32, h * w * bands)[:] = (c + c * coef).reshape(-1)


for _name, _fn in list(globals().items()):
    if _name.startswith("_k_"):
        setattr(EmuBackend, _name[1:], _fn)
