"""GPU: the four scene-preparation launches of csrc/scene.hip against NumPy -- the rank select and the extrema
exactly, the prepared scene bit for bit, the masked sums within fp64 summation error and identical between runs."""
import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import OUT_DTYPES, SCENE_RANK_WS_WORDS, Ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


def up(be, a):
    return be.upload(np.ascontiguousarray(a).reshape(-1).view(np.uint8))


def geometry(view, root):
    """(h, w, bands, sy, sx, sb, byte offset) of a 3-d view into the contiguous array `root`"""
    item = view.dtype.itemsize
    off = view.__array_interface__["data"][0] - root.__array_interface__["data"][0]
    return tuple(int(v) for v in view.shape) + tuple(int(s) // item for s in view.strides) + (off,)


def sources(rng, dtype, h, w, bands):
    """the same logical [h, w, bands] scene stored chunky and as a window of a [band, column, row] file"""
    if np.dtype(dtype).kind == "f":
        scene = ((rng.random((h, w, bands)) - 0.3) * 5000).astype(dtype)  # negative floats too
    else:
        info = np.iinfo(dtype)
        scene = rng.integers(info.min, int(info.max) + 1, (h, w, bands)).astype(dtype)
    yield "chunky", scene, scene
    stored = np.zeros((bands + 2, w, h + 7), dtype)
    stored[1:-1, :, 3:-4] = scene.transpose(2, 1, 0)
    yield "swapped", np.swapaxes(stored[1:-1, :, 3:-4], 0, 2), stored


# ------------------------------------------------------------------------------------------------ rank select
def rank_select(be, view, root, lo, hi):
    h, w, bands, sy, sx, sb, off = geometry(view, root)
    src = up(be, root)
    out = be.zeros(4 * bands, torch.uint8)
    ws = be.empty(bands * SCENE_RANK_WS_WORDS * 4, torch.uint8)
    be.call("scene_rank_select_u16", Ref(src, off), h, w, bands, sy, sx, sb, lo, hi, Ref(out), Ref(out, 2 * bands),
            Ref(ws))
    got = out.cpu().numpy().view(np.uint16)
    return got[:bands], got[bands:]


@pytest.mark.parametrize("bands", [1, 7, 65])
@pytest.mark.parametrize("pixels", [1, 255, 4097])
def test_rank_select(be, bands, pixels):
    rng = np.random.default_rng(bands * 10000 + pixels)
    h = 17 if pixels == 255 else (241 if pixels == 4097 else 1)  # 255 = 17 x 15, 4097 = 241 x 17
    w = pixels // h
    assert h * w == pixels
    n = pixels
    scene = rng.integers(0, 65536, (h, w, bands)).astype(np.uint16)
    if bands > 1:
        scene[..., 0] = 777  # an all-equal band
    if bands > 2:
        scene[..., 1] = rng.integers(0, 40, (h, w))  # few distinct values: long runs inside one bucket
        flat = scene[..., 2].reshape(-1)
        flat[:] = np.where(np.arange(n) < (n + 1) // 2, 255, 256)  # the middle ranks straddle a high-byte bucket
        rng.shuffle(flat)
    if bands > 3 and n > 1:
        scene[..., 3].reshape(-1)[:2] = [0, 65535]
    ranks = {(0, 0), (n - 1, n - 1), (0, n - 1), ((n - 1) // 2, min((n - 1) // 2 + 1, n - 1)),
             (int(0.95 * (n - 1)), min(int(0.95 * (n - 1)) + 1, n - 1))}
    stored = np.zeros((bands, w, h + 5), np.uint16) + 60000
    stored[:, :, 2:-3] = scene.transpose(2, 1, 0)
    srt = np.sort(scene.reshape(n, bands), axis=0)
    for lo, hi in sorted(ranks):
        for view, root in ((scene, scene), (np.swapaxes(stored[:, :, 2:-3], 0, 2), stored)):
            got_lo, got_hi = rank_select(be, view, root, lo, hi)
            assert np.array_equal(got_lo, srt[lo]) and np.array_equal(got_hi, srt[hi]), (lo, hi)
    if bands > 2 and n > 1:
        lo = (n - 1) // 2
        assert (srt[lo, 2], srt[lo + 1, 2]) == (255, 256)
    if bands > 3 and n > 1:
        assert srt[0, 3] == 0 and srt[-1, 3] == 65535


@pytest.mark.parametrize("kind", ["random", "straddle", "extremes", "equal"])
def test_rank_select_one_band(be, kind):
    """a one-band raster is fetched along the pixels and counted by one lane: every value pattern on that path"""
    rng = np.random.default_rng(41)
    h, w = 241, 17
    n = h * w
    flat = rng.integers(0, 65536, n).astype(np.uint16)
    if kind == "straddle":
        flat = np.where(np.arange(n) < (n + 1) // 2, 255, 256).astype(np.uint16)
        rng.shuffle(flat)
    elif kind == "extremes":
        flat[:3] = [0, 65535, 65535]
    elif kind == "equal":
        flat[:] = 40000
    scene = flat.reshape(h, w, 1)
    srt = np.sort(flat)
    mid = (n - 1) // 2
    for lo, hi in ((0, 0), (n - 1, n - 1), (0, n - 1), (mid, mid + 1), (int(0.95 * (n - 1)), int(0.95 * (n - 1)) + 1)):
        got_lo, got_hi = rank_select(be, scene, scene, lo, hi)
        assert (int(got_lo[0]), int(got_hi[0])) == (int(srt[lo]), int(srt[hi])), (lo, hi)
    if kind == "straddle":
        assert (srt[mid], srt[mid + 1]) == (255, 256)


# ------------------------------------------------------------------------------------------------ extrema, prepare
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16, np.float32])
@pytest.mark.parametrize("shape", [(3, 4, 5), (23, 70, 67), (130, 3, 1)])
def test_extrema(be, dtype, shape):
    rng = np.random.default_rng(5)
    for layout, view, root in sources(rng, dtype, *shape):
        h, w, bands, sy, sx, sb, off = geometry(view, root)
        item = view.dtype.itemsize
        src = up(be, root)
        clip = np.sort(view.reshape(-1, bands), axis=0)[int(0.8 * (h * w - 1))].astype(dtype)
        sub = view.min(axis=(0, 1)) + np.asarray(3, dtype)  # above the minimum: the integer subtraction wraps
        for use_clip, use_sub in ((False, False), (True, False), (False, True), (True, True)):
            out = be.zeros(2 * bands * item, torch.uint8)
            ws = be.empty(2 * 64 * bands * item, torch.uint8)
            be.call("scene_extrema", Ref(src, off), OUT_DTYPES[view.dtype], h, w, bands, sy, sx, sb,
                    Ref(up(be, clip)) if use_clip else None, Ref(up(be, sub)) if use_sub else None, Ref(out),
                    Ref(out, bands * item), Ref(ws), 64)
            got = out.cpu().numpy().view(dtype)
            v = np.minimum(view, clip) if use_clip else view
            v = (v - sub).astype(dtype) if use_sub else v
            assert np.array_equal(got[:bands], v.min(axis=(0, 1))), (layout, use_clip, use_sub)
            assert np.array_equal(got[bands:], v.max(axis=(0, 1))), (layout, use_clip, use_sub)


def prepare(be, view, root, pad, clip, lo, scale):
    h, w, bands, sy, sx, sb, off = geometry(view, root)
    out = be.empty((h + 2 * pad) * (w + 2 * pad) * bands, torch.float32)
    keep = [up(be, root)] + [None if a is None else up(be, a) for a in (clip, lo, scale)]
    be.call("scene_prepare_f32", Ref(keep[0], off), OUT_DTYPES[view.dtype], h, w, bands, sy, sx, sb, pad,
            *[None if t is None else Ref(t) for t in keep[1:]], Ref(out))
    return out.cpu().numpy().reshape(h + 2 * pad, w + 2 * pad, bands)


def prepare_ref(view, pad, clip, lo, scale):
    v = view if clip is None else np.minimum(view, clip)
    v = v if lo is None else (v - lo).astype(view.dtype)
    v = np.pad(v, ((pad, pad), (pad, pad), (0, 0)), mode="symmetric").astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v if scale is None else v / scale


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16, np.float32])
@pytest.mark.parametrize("pad", [0, 1, 5])
def test_prepare_small_scene(be, dtype, pad):
    """3 x 4 pixels: with pad 5 the reflection wraps around the scene more than once"""
    rng = np.random.default_rng(11 + pad)
    for layout, view, root in sources(rng, dtype, 3, 4, 6):
        bands = 6
        lo = view.min(axis=(0, 1))
        lo[1] = lo[1] + np.asarray(2, dtype)  # some samples below the offset: integers wrap, as NumPy's do
        clip = np.sort(view.reshape(-1, bands), axis=0)[8].astype(dtype)
        scale = (rng.random(bands) * 3000 + 7).astype(np.float32)  # no powers of two: the division must round
        scale[2] = 0.0  # a zero-scale band: inf and, where the numerator is 0, nan
        view[0, 0, 2] = lo[2]
        for use_clip in (False, True):
            for c, l, s in ((clip if use_clip else None, lo, scale), (clip if use_clip else None, None, None),
                            (None, lo, None)):
                got = prepare(be, view, root, pad, c, l, s)
                want = prepare_ref(view, pad, c, l, s)
                assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
                    (layout, use_clip, l is None, s is None)
        assert np.isnan(prepare_ref(view, pad, None, lo, scale)[..., 2]).any()


@pytest.mark.parametrize("dtype,shape,pad", [(np.uint16, (70, 131, 67), 3), (np.float32, (33, 65, 130), 2),
                                             (np.float32, (129, 66, 1), 4), (np.uint16, (65, 9, 12), 2)])
def test_prepare_many_tiles(be, dtype, shape, pad):
    """more than one pixel tile and band tile, no extent a multiple of the 64 x 64 tile; one LiDAR-shaped case"""
    rng = np.random.default_rng(2)
    for layout, view, root in sources(rng, dtype, *shape):
        bands = shape[2]
        lo = view.min(axis=(0, 1))
        scale = (view.max(axis=(0, 1)) - lo).astype(dtype).astype(np.float32)
        got = prepare(be, view, root, pad, None, lo, scale)
        want = prepare_ref(view, pad, None, lo, scale)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), layout


# ------------------------------------------------------------------------------------------------ masked sums
@pytest.mark.parametrize("shape", [(9, 11, 5), (40, 53, 67), (300, 301, 12)])
def test_masked_sums(be, shape):
    hp, wp, bands = shape
    rng = np.random.default_rng(8)
    scene = ((rng.random(shape) - 0.2) * 3).astype(np.float32)
    for kind in ("mixed", "all lit", "all shadow"):
        smap = {"mixed": (rng.random((hp, wp)) < 0.3), "all lit": np.zeros((hp, wp), bool),
                "all shadow": np.ones((hp, wp), bool)}[kind].astype(np.uint8)
        runs = []
        for _ in range(2):
            out = be.zeros((2 * bands + 2) * 8, torch.uint8)
            ws = be.empty(256 * 2 * (bands + 1) * 8, torch.uint8)
            be.call("scene_masked_sums", Ref(up(be, scene).view(torch.float32)), Ref(up(be, smap)), hp, wp, bands,
                    Ref(out), Ref(out, 2 * bands * 8), Ref(ws), 256)
            runs.append(out.cpu().numpy().copy())
        assert np.array_equal(runs[0], runs[1]), "two runs, identical bits"
        sums = runs[0][:2 * bands * 8].view(np.float64).reshape(2, bands)
        counts = runs[0][2 * bands * 8:].view(np.int64)
        on = smap != 0
        assert counts.tolist() == [int(on.sum()), int((~on).sum())]
        s64 = scene.astype(np.float64)
        for k, mask in enumerate((on, ~on)):
            exact = np.asarray([float(np.sum(s64[..., b][mask])) for b in range(bands)])
            mag = np.asarray([float(np.sum(np.abs(s64[..., b][mask]))) for b in range(bands)])
            # fp64 sums of n < 2^24 float32 values: |error| <= n * 2^-53 * sum|x| in any order (both sides)
            assert np.all(np.abs(sums[k] - exact) <= 2 * mask.sum() * 2.0 ** -53 * mag)
            if mask.sum() == 0:
                assert np.all(sums[k] == 0)
        if kind == "mixed":
            with np.errstate(all="ignore"):
                ratio = ((sums[1] / counts[1]) / (sums[0] / counts[0])).astype(np.float32)
            exact = s64[~on].mean(axis=0) / s64[on].mean(axis=0)
            assert np.all(np.abs(ratio.astype(np.float64) - exact) <= 2.0 ** -23 * np.abs(exact))
