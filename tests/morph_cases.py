"""TEST INFRASTRUCTURE: inputs, the brute-force reference and the launch runners for the grey-scale morphology entry
points (include/hypel.h, hypel_morph_*) and MorphologicalProfile, shared by tests/test_morph_emu.py (NumPy twin) and
tests/test_gpu_morph.py (device).

The reference works on keys, literally as the header defines the operators: the image shifted once per offset of the
structuring element, minimum / maximum taken offset by offset, offsets outside the raster skipped; the reconstruction is
the one-pixel step m <- min(dilate3x3(m), mask) iterated from min(marker, mask) until nothing changes.  Every comparison
in the tests is numpy.array_equal on bits: there is no tolerance anywhere."""
import functools

import numpy as np
import torch

from hypelcnn_amd.backend import MORPH_DILATE, MORPH_DISK, MORPH_ERODE, MORPH_SQUARE, Ref

SENTINEL = 0x5A
SHAPES = {"disk": MORPH_DISK, "square": MORPH_SQUARE}
OPS = {"erode": MORPH_ERODE, "dilate": MORPH_DILATE}
RADII = (0, 1, 2, 7, 32)
# h, w over {1, 2, 15, 16, 17, 63, 64, 65, 130} (around the 64 x 16 tile), paired sparsely: every value occurs as a
# height and as a width; c over {1, 3, 5} along the pairs
SIZES = ((1, 1, 3), (1, 130, 5), (2, 17, 1), (15, 64, 3), (16, 16, 5), (17, 65, 1), (63, 2, 3), (64, 63, 5), (65, 15, 1),
         (130, 1, 3), (130, 65, 1))
VALUES = ("normal", "plateau", "special")


# ------------------------------------------------------------------------------------------------------- keys, bits
def keys_of(x):
    """float32 array -> uint32 keys (include/hypel.h: k = (u >> 31) ? ~u : (u | 0x80000000))"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> np.uint32(31) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def floats_of(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k >> np.uint32(31) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------------------------------------------- inputs
def image(kind, h, w, c, seed=0):
    """float32 [h, w, c]: random normals; a plateau image of few distinct values; or one that holds -0 / +0 side by
    side, +-inf, denormals and NaNs of both signs (with payloads) among normals"""
    rng = np.random.default_rng([seed, h, w, c, VALUES.index(kind)])
    if kind == "normal":
        return rng.standard_normal((h, w, c)).astype(np.float32)
    if kind == "plateau":
        return rng.integers(0, 4, (h, w, c)).astype(np.float32) * np.float32(0.5) - np.float32(0.5)
    x = rng.standard_normal((h, w, c)).astype(np.float32)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7FC00000,
                        0xFFC00000, 0x7FC12345, 0xFFA54321, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32).view(np.float32)
    pick = rng.integers(0, 2 * len(special), (h, w, c))
    x = np.where(pick < len(special), special[pick % len(special)], x)
    flat = x.reshape(-1)
    flat[0::7] = np.float32(-0.0)  # -0 and +0 side by side
    flat[1::7] = np.float32(0.0)
    return flat.reshape(h, w, c)


def layouts(x):
    """The same image as (name, float32 buffer, origin in floats, stride_y, stride_x): dense, and the interior of a
    padded, NaN-filled scene [h + 4][w + 4][c + 1] (a trailing channel that is never read) that starts one float into
    its buffer, so that the origin is 4-byte aligned only."""
    h, w, c = x.shape
    yield "dense", x.reshape(-1).copy(), 0, w * c, c
    scene = np.full((h + 4, w + 4, c + 1), np.float32(np.nan))
    scene[2:2 + h, 2:2 + w, :c] = x
    buf = np.concatenate([np.full(1, np.nan, np.float32), scene.reshape(-1)])
    yield "padded", buf, 1 + 2 * (w + 4 + 1) * (c + 1), (w + 4) * (c + 1), c + 1


def serpentine(h, w):
    """(marker, mask) float32 [h, w, 1]: a one-pixel corridor on the even rows, joined by one pixel at alternating ends of
    the odd rows; the mask is 1 on the corridor and 0 beside it, the marker 1 at the corridor's first pixel only.  The
    limit fills the whole corridor, along a path of about h * w / 2 pixels."""
    mask = np.zeros((h, w, 1), np.float32)
    mask[0::2] = 1.0
    for y in range(1, h, 2):
        mask[y, w - 1 if (y // 2) % 2 == 0 else 0] = 1.0
    marker = np.zeros((h, w, 1), np.float32)
    marker[0, 0] = 1.0
    return marker, mask


# ------------------------------------------------------------------------------------------------------- reference
def offsets(radius, shape):
    span = range(-radius, radius + 1)
    if shape == "square":
        return [(dy, dx) for dy in span for dx in span]
    return [(dy, dx) for dy in span for dx in span if dy * dy + dx * dx <= radius * radius]


def ref_erode_dilate(k, radius, shape, op):
    """keys [h, w, c] -> keys: shifted minimum / maximum over the element's offsets, offsets outside the raster skipped"""
    h, w, _ = k.shape
    take = np.minimum if op == "erode" else np.maximum
    acc = k.copy()
    for dy, dx in offsets(radius, shape):
        ys, yd = slice(max(0, dy), min(h, h + dy)), slice(max(0, -dy), min(h, h - dy))
        xs, xd = slice(max(0, dx), min(w, w + dx)), slice(max(0, -dx), min(w, w - dx))
        if ys.start >= ys.stop or xs.start >= xs.stop:
            continue
        acc[yd, xd] = take(acc[yd, xd], k[ys, xs])
    return acc


def ref_step(m, mask, method):
    """one one-pixel step of a clamped marker: min(dilate3x3(m), mask), or the dual"""
    if method == "dilation":
        return np.minimum(ref_erode_dilate(m, 1, "square", "dilate"), mask)
    return np.maximum(ref_erode_dilate(m, 1, "square", "erode"), mask)


def ref_reconstruct(marker, mask, method):
    """keys -> (the limit, one-pixel steps it took)"""
    clamp = np.minimum if method == "dilation" else np.maximum
    m = clamp(marker, mask)
    for steps in range(marker.shape[0] * marker.shape[1] + 2):
        nxt = ref_step(m, mask, method)
        if np.array_equal(nxt, m):
            return m, steps
        m = nxt
    raise AssertionError("the reference reconstruction did not settle")


def ref_opening(k, radius, shape, by_reconstruction=True):
    eroded = ref_erode_dilate(k, radius, shape, "erode")
    return ref_reconstruct(eroded, k, "dilation")[0] if by_reconstruction else ref_erode_dilate(eroded, radius, shape, "dilate")


def ref_closing(k, radius, shape, by_reconstruction=True):
    dilated = ref_erode_dilate(k, radius, shape, "dilate")
    return ref_reconstruct(dilated, k, "erosion")[0] if by_reconstruction else ref_erode_dilate(dilated, radius, shape, "erode")


def ref_profile(x, radii, shape="disk", by_reconstruction=True):
    """float32 [h, w, c] -> float32 [h, w, c (2 S + 1)]: base b at channels b (2 S + 1) ..: [phi_rS .. phi_r1, f, gamma_r1
    .. gamma_rS]"""
    k = keys_of(x)
    h, w, c = k.shape
    levels = [ref_closing(k, r, shape, by_reconstruction) for r in reversed(radii)] + [k] + \
             [ref_opening(k, r, shape, by_reconstruction) for r in radii]
    return floats_of(np.stack(levels, axis=3).reshape(h, w, c * len(levels)))


@functools.lru_cache(maxsize=None)
def erode_dilate_case(kind, h, w, c, radius, shape, op):
    """(input float32 [h, w, c], expected keys) -- computed once per process and left unchanged"""
    x = image(kind, h, w, c)
    want = ref_erode_dilate(keys_of(x), radius, shape, op)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


# ------------------------------------------------------------------------------------------------------- runners
def guarded(be, count, dtype=torch.int32):
    """a device buffer of `count` 4-byte items between two 64-byte guards of SENTINEL bytes, itself filled with SENTINEL,
    as (tensor of the items, check that the guards are intact)"""
    raw = be.upload(np.full(128 + count * 4, SENTINEL, np.uint8))
    body = raw[64:64 + count * 4].view(dtype)

    def intact():
        host = raw.cpu().numpy()
        return bool((host[:64] == SENTINEL).all() and (host[64 + count * 4:] == SENTINEL).all())
    return body, intact


def host_keys(t):
    return t.cpu().numpy().view(np.uint32).copy()


def upload_keys(be, k):
    return be.upload(np.ascontiguousarray(k, dtype=np.uint32).view(np.int32))


def run_keys(be, buf, origin, h, w, c, stride_y, stride_x):
    keys, intact = guarded(be, h * w * c)
    be.call("morph_keys_u32", Ref(be.upload(buf), origin), h, w, c, stride_y, stride_x, Ref(keys))
    out = host_keys(keys).reshape(h, w, c)
    assert intact()
    return out, keys


def run_erode_dilate(be, keys_d, h, w, c, radius, shape, op):
    out, intact = guarded(be, h * w * c)
    be.call("morph_erode_dilate_u32", Ref(keys_d), h, w, c, radius, SHAPES[shape], OPS[op], Ref(out))
    got = host_keys(out).reshape(h, w, c)
    assert intact()
    return got


def run_sweep(be, marker, mask, method, flag=0):
    """one launch on key images -> (marker_out, the changed word afterwards)"""
    h, w, c = marker.shape
    out, intact = guarded(be, h * w * c)
    changed, flag_intact = guarded(be, 1)
    changed.copy_(torch.tensor([flag], dtype=torch.int32))
    be.call("morph_reconstruct_sweep_u32", Ref(upload_keys(be, marker)), Ref(upload_keys(be, mask)), h, w, c,
            MORPH_DILATE if method == "dilation" else MORPH_ERODE, Ref(out), Ref(changed))
    got = host_keys(out).reshape(h, w, c)
    word = int(changed.cpu()[0])
    assert intact() and flag_intact()
    return got, word


def check_sweep_contract(marker, mask, method, out, word, limit):
    """the four clauses of include/hypel.h for one launch that started with *changed == 0"""
    lo, hi = (np.minimum(marker, mask), limit) if method == "dilation" else (limit, np.maximum(marker, mask))
    assert (out >= lo).all() and (out <= hi).all()
    same = np.array_equal(out, marker)
    assert same == np.array_equal(marker, limit)
    assert word == (0 if same else 1)


def run_store(be, k, pad, out_c, chan_offset, chan_step):
    """-> the whole padded stack as uint32 [h + 2 pad][w + 2 pad][out_c], pre-filled with SENTINEL bytes"""
    h, w, c = k.shape
    hp, wp = h + 2 * pad, w + 2 * pad
    out, intact = guarded(be, hp * wp * out_c, torch.float32)
    be.call("morph_profile_store_f32", Ref(upload_keys(be, k)), h, w, c, pad, Ref(out), out_c, chan_offset, chan_step)
    got = out.cpu().numpy().view(np.uint32).copy().reshape(hp, wp, out_c)
    assert intact()
    return got
