"""TEST INFRASTRUCTURE: NumPy twins of the grey-scale morphology entry points (include/hypel.h, hypel_morph_*), attached to
tests/emu_backend.EmuBackend on import.  Written from the header.  Every launch is appended to the backend's `launch_log`.

What the twins promise: the argument checks of the entry points (an assertion where the library answers "invalid
argument") and the header's values BIT FOR BIT -- everything is integer min / max on keys, nothing rounds.  How they get
there is their own: the structuring element is one row window per dy, each the reduction of two overlapping power-of-two
windows from doubling tables of an image padded with the operation's identity (the reference of tests/morph_cases.py
shifts the image once per offset), and a sweep is
ONE one-pixel Jacobi step of the clamped marker, which the header's contract allows: it advances a front by a pixel where
the kernel advances it by a tile, so the emulated driver needs more sweeps for the same limit."""
import numpy as np

from hypelcnn_amd.backend import MORPH_DILATE, MORPH_DISK, MORPH_ERODE, MORPH_MAX_RADIUS, MORPH_SQUARE
from tests.emu_backend import EmuBackend, _arr

LIMIT = 1 << 40
SIDE = (1 << 31) - 1
TOP = np.uint32(0xFFFFFFFF)


def _image_ok(h, w, c):
    assert 1 <= h <= SIDE and 1 <= w <= SIDE and c >= 1 and h * w * c <= LIMIT


def _image(ref, h, w, c):
    """the dense key image behind a Ref as a uint32 [h][w][c] view"""
    assert ref is not None
    a = _arr(ref, np.uint32)
    assert a.size >= h * w * c, "the image leaves its buffer"
    return a[:h * w * c].reshape(h, w, c)


def _k_morph_keys_u32(self, x, h, w, c, stride_y, stride_x, keys):
    self.launch_log.append("morph_keys_u32")
    assert x is not None and keys is not None
    _image_ok(h, w, c)
    assert c <= stride_y <= LIMIT and c <= stride_x <= LIMIT
    a = _arr(x)
    span = (h - 1) * stride_y + (w - 1) * stride_x + c
    assert span <= a.size, "the view leaves its buffer"
    out = _image(keys, h, w, c)
    assert not np.shares_memory(a[:span], out)
    u = np.ascontiguousarray(np.lib.stride_tricks.as_strided(a.view(np.uint32), shape=(h, w, c),
                                                             strides=(stride_y * 4, stride_x * 4, 4)))
    out[...] = np.where(u >> np.uint32(31) != 0, ~u, u | np.uint32(0x80000000))


def _half_width(radius, shape, dy):
    if shape == MORPH_SQUARE:
        return radius
    s = 0
    while (s + 1) ** 2 <= radius * radius - dy * dy:
        s += 1
    return s


def _k_morph_erode_dilate_u32(self, src, h, w, c, radius, shape, op, dst):
    self.launch_log.append("morph_erode_dilate_u32")
    _image_ok(h, w, c)
    assert 0 <= radius <= MORPH_MAX_RADIUS and shape in (MORPH_DISK, MORPH_SQUARE) and op in (MORPH_ERODE, MORPH_DILATE)
    a, out = _image(src, h, w, c), _image(dst, h, w, c)
    assert not np.shares_memory(a, out)
    reduce_, identity = (np.minimum, TOP) if op == MORPH_ERODE else (np.maximum, np.uint32(0))
    padded = np.full((h + 2 * radius, w + 2 * radius, c), identity, np.uint32)
    padded[radius:radius + h, radius:radius + w] = a
    # tables[j][:, i] = the reduction of padded[:, i : i + 2^j]; a window of any length is two of them that overlap
    tables = [padded]
    while 2 ** len(tables) <= 2 * radius + 1:
        half = 2 ** (len(tables) - 1)
        tables.append(reduce_(tables[-1][:, :-half], tables[-1][:, half:]))
    acc = np.full((h, w, c), identity, np.uint32)
    for dy in range(-radius, radius + 1):
        s = _half_width(radius, shape, dy)
        length = 2 * s + 1
        j = length.bit_length() - 1
        rows = tables[j][radius + dy:radius + dy + h]
        first, second = radius - s, radius - s + length - 2 ** j
        acc = reduce_(acc, reduce_(rows[:, first:first + w], rows[:, second:second + w]))
    out[...] = acc


def _k_morph_reconstruct_sweep_u32(self, marker_in, mask, h, w, c, op, marker_out, changed):
    self.launch_log.append("morph_reconstruct_sweep_u32")
    _image_ok(h, w, c)
    assert op in (MORPH_ERODE, MORPH_DILATE) and changed is not None
    m, k, out = _image(marker_in, h, w, c), _image(mask, h, w, c), _image(marker_out, h, w, c)
    assert not np.shares_memory(m, out) and not np.shares_memory(k, out)
    spread, clamp, identity = (np.maximum, np.minimum, np.uint32(0)) if op == MORPH_DILATE else (np.minimum, np.maximum, TOP)
    padded = np.full((h + 2, w + 2, c), identity, np.uint32)
    padded[1:h + 1, 1:w + 1] = clamp(m, k)
    result = padded[1:h + 1, 1:w + 1].copy()
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            spread(result, padded[dy:dy + h, dx:dx + w], out=result)
    clamp(result, k, out=result)
    if not np.array_equal(result, m):
        _arr(changed, np.int32)[0] = 1
    out[...] = result


def _k_morph_profile_store_f32(self, keys, h, w, c, pad, out, out_c, chan_offset, chan_step):
    self.launch_log.append("morph_profile_store_f32")
    _image_ok(h, w, c)
    assert 0 <= pad <= min(h, w) and out_c >= 1 and chan_offset >= 0 and chan_step >= 1
    assert chan_offset + (c - 1) * chan_step < out_c and (h + 2 * pad) * (w + 2 * pad) * out_c <= LIMIT
    k = _image(keys, h, w, c)
    stack = _image(out, h + 2 * pad, w + 2 * pad, out_c)
    assert not np.shares_memory(k, stack)
    u = np.where(k >> np.uint32(31) != 0, k & np.uint32(0x7FFFFFFF), ~k)
    stack[:, :, chan_offset:chan_offset + (c - 1) * chan_step + 1:chan_step] = np.pad(u, ((pad, pad), (pad, pad), (0, 0)),
                                                                                    mode="symmetric")


EmuBackend.k_morph_keys_u32 = _k_morph_keys_u32
EmuBackend.k_morph_erode_dilate_u32 = _k_morph_erode_dilate_u32
EmuBackend.k_morph_reconstruct_sweep_u32 = _k_morph_reconstruct_sweep_u32
EmuBackend.k_morph_profile_store_f32 = _k_morph_profile_store_f32
