"""TEST INFRASTRUCTURE: the stored orders, extents and strides the scene-preparation launches (include/hypel.h,
hypel_scene_*, hypel_shadow_correct_f32) are asked to read in place, their plain NumPy references and one runner per
launch, shared by tests/test_scene_layout_cases_emu.py (NumPy twin) and tests/test_gpu_scene_layouts.py (device).

VIEWS.  A logical [h, w, bands] scene in each of its six stored orders, every one a window of a larger C-contiguous
root: the first item at an odd element offset, a gap before and after the window on every stored axis.  The scene's
values lie strictly inside the dtype's range and the gaps alternate between the dtype's lowest and highest value, so
ONE sample fetched from a gap moves an extremum, a rank-0 or rank-(n - 1) value or a prepared pixel.  Axes of extent 1
are passed with stride 0, as device_scene.resident_view reports them.  Three more kinds of view only as_strided can make
(the header admits any stride >= 0): pixels and bands that overlap (sx == sb == 1) at 15 and at 16 bands -- the two
sides of the kernel's tie rule -- and a zero stride on each axis in turn, at an extent above 1.

SHAPES.  (66, 70, 67): both pixel extents past one 64-position tile with a ragged tail, two 64-band tiles, three
32-band tiles of the rank histogram; and every way of setting extents of it to 1.

REFERENCES.  NumPy's own arithmetic on the view itself: numpy.minimum, the source dtype's wrapping subtraction, min and
max over axes (0, 1), numpy.sort(...)[rank], numpy.pad(mode="symmetric") -> astype(float32) -> true division, and the
float32 correction expression of tests/test_components_emu.numpy_correction.  Every comparison is bit for bit.

RUNNERS.  run_*(be, view, runs): the launch through be.call, outputs and workspaces cut from ONE allocation filled with
a sentinel byte (so the workspaces are exactly as long as the header asks, arrive dirty, and a write outside any buffer
is seen); each launch is issued `runs` times and must give equal bits."""
import functools

import numpy as np
import torch
from numpy.lib.stride_tricks import as_strided

from hypelcnn_amd.backend import OUT_DTYPES, SCENE_RANK_WS_WORDS, Ref

ORDERS = ("hwb", "hbw", "whb", "wbh", "bhw", "bwh")
FULL = (66, 70, 67)
SHAPES = (FULL, (1, 70, 67), (66, 1, 67), (66, 70, 1), (1, 1, 67), (1, 70, 1), (66, 1, 1), (1, 1, 1))
DTYPES = (np.uint8, np.uint16, np.int16, np.float32)
GAP_BEFORE, GAP_AFTER = 1, 2
SENTINEL = 0x5A
GUARD = 64
TILE = 64  # positions of a pixel tile (csrc/scene.hip)


def limits(dtype):
    dt = np.dtype(dtype)
    info = np.finfo(dt) if dt.kind == "f" else np.iinfo(dt)
    return dt.type(info.min), dt.type(info.max)


def draw(rng, dtype, shape):
    """values strictly inside the dtype's range (floats of both signs)"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return ((rng.random(shape) - 0.3) * 5000).astype(dt)
    lo, hi = limits(dt)
    return rng.integers(int(lo) + 1, int(hi), shape).astype(dt)  # lo + 1 .. hi - 1


def gap_filled(count, dtype):
    root = np.empty(count, dtype)
    root[0::2], root[1::2] = limits(dtype)
    return root


class View:
    """view: the [h, w, bands] NumPy view; root: the flat C-contiguous array it lies in; offset: its first item in root
    (elements); strides: element strides as the launches get them; key: what its values depend on"""

    def __init__(self, name, view, root, key):
        item = view.dtype.itemsize
        self.name, self.view, self.root, self.key = name, view, root, key
        self.offset = (view.__array_interface__["data"][0] - root.__array_interface__["data"][0]) // item
        self.strides = tuple(0 if n == 1 else int(s) // item for n, s in zip(view.shape, view.strides))
        last = self.offset + sum((n - 1) * s for n, s in zip(view.shape, self.strides))
        assert root.ndim == 1 and root.flags.c_contiguous and 0 <= self.offset and last < root.size
        view.setflags(write=False)
        root.setflags(write=False)

    @property
    def geometry(self):
        return tuple(int(n) for n in self.view.shape) + self.strides

    def __repr__(self):
        return f"{self.name} {self.view.dtype} {self.geometry}"


def windowed(scene, order, key):
    """the scene stored in `order` (slowest axis first) as a window of a larger root"""
    axes = ["hwb".index(c) for c in order]  # stored axis i holds logical axis axes[i]
    stored = [scene.shape[a] for a in axes]
    padded = [n + GAP_BEFORE + GAP_AFTER for n in stored]
    first = GAP_BEFORE * (padded[1] * padded[2] + padded[2] + 1)
    lead = 1 if first % 2 == 0 else 2
    root = gap_filled(lead + int(np.prod(padded)), scene.dtype)
    window = root[lead:].reshape(padded)[tuple(slice(GAP_BEFORE, GAP_BEFORE + n) for n in stored)]
    window[...] = scene.transpose(axes)
    out = View(f"{order}{scene.shape}", window.transpose(np.argsort(axes)), root, key)
    assert out.offset % 2 == 1 and np.array_equal(out.view, scene)
    return out


def overlapping(dtype, bands):
    """sx == sb == 1: sample (y, x, b) is item y * 101 + x + b of the rows' data; between the rows lie gaps"""
    h, w, sy, lead = 5, 70, 101, 3
    rng = np.random.default_rng([11, np.dtype(dtype).num, bands])
    root = gap_filled(lead + h * sy, dtype)
    for y in range(h):
        root[lead + y * sy:lead + y * sy + w + bands - 1] = draw(rng, dtype, w + bands - 1)
    item = root.itemsize
    view = as_strided(root[lead:], (h, w, bands), (sy * item, item, item))
    return View(f"overlap{(h, w, bands)}", view, root, ("overlap", bands))


def zero_stride(dtype, axis, order):
    shape = (5, 70, 35)
    rng = np.random.default_rng([13, np.dtype(dtype).num, axis])
    base = windowed(draw(rng, dtype, shape), order, None)
    strides = list(base.view.strides)
    strides[axis] = 0
    view = as_strided(base.view, shape, strides)
    return View(f"zero_s{'yxb'[axis]}_{order}{shape}", view, base.root, ("zero", axis))


@functools.lru_cache(maxsize=None)
def scene(dtype, shape):
    a = draw(np.random.default_rng([7, np.dtype(dtype).num, *shape]), dtype, shape)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def window_views(dtype, shape=FULL):
    """the six stored orders of scene(dtype, shape)"""
    return tuple(windowed(scene(dtype, shape), order, ("window", shape)) for order in ORDERS)


@functools.lru_cache(maxsize=None)
def strided_views(dtype):
    return (overlapping(dtype, 15), overlapping(dtype, 16), zero_stride(dtype, 0, "hwb"), zero_stride(dtype, 1, "bhw"),
            zero_stride(dtype, 2, "whb"))


def views(dtype):
    """the whole case table of one dtype: 8 shapes x 6 orders, then the five as_strided views"""
    for shape in SHAPES:
        yield from window_views(dtype, shape)
    yield from strided_views(dtype)


def fetch_path(h, w, bands, sy, sx, sb):
    """csrc/scene.hip make_geom restated, for the coverage assertion below and the summaries only: (y_fast, band_fast)"""
    far = 2 ** 63 - 1
    ey, ex, eb = (far if n == 1 else s for n, s in ((h, sy), (w, sx), (bands, sb)))
    y_fast = ey < ex
    ef = ey if y_fast else ex
    return int(y_fast), int(eb < ef or (eb == ef and bands >= 16))


def coverage(dtype=np.uint8):
    """{(y_fast, band_fast, axes of extent 1): [view names]} of the case table"""
    table = {}
    for v in views(dtype):
        ones = "".join(c for c, n in zip("hwb", v.view.shape) if n == 1)
        table.setdefault(fetch_path(*v.geometry) + (ones,), []).append(v.name)
    return table


_many_bands = {k[:2] for k in coverage() if "b" not in k[2]}
assert _many_bands == {(0, 0), (0, 1), (1, 0), (1, 1)}, _many_bands
assert {fetch_path(*v.geometry) for v in strided_views(np.uint8)[:2]} == {(0, 0), (0, 1)}  # the tie, both sides


# ----------------------------------------------------------------------------------------------------- plumbing
def up(be, a):
    return be.upload(np.ascontiguousarray(a).reshape(-1).view(np.uint8))


def source(be, v):
    """(Ref of the first item, the launches' geometry arguments); the root is uploaded as it is"""
    return Ref(up(be, v.root), v.offset * v.root.itemsize), v.geometry


class Guarded:
    """byte buffers of the given sizes in one device allocation, GUARD or more sentinel bytes around each; the buffers
    themselves hold the sentinel too until a launch writes them"""

    def __init__(self, be, *sizes):
        self.spans, pos = [], GUARD
        for n in sizes:
            self.spans.append((pos, int(n)))
            pos += int(n)
            pos += GUARD + (-pos) % 16
        self.raw = be.empty(pos, torch.uint8)
        self.raw.fill_(SENTINEL)

    def ref(self, i, byte_off=0):
        return Ref(self.raw, self.spans[i][0] + byte_off)

    def fetch(self, *which):
        """the buffers `which` as bytes, after checking every byte outside all buffers"""
        host = self.raw.cpu().numpy()
        pos = 0
        for p, n in self.spans + [(host.size, 0)]:
            assert (host[pos:p] == SENTINEL).all(), "a launch wrote outside its buffers"
            pos = p + n
        return [host[self.spans[i][0]:self.spans[i][0] + self.spans[i][1]].copy() for i in which]


def issue(launch, runs):
    """launch() -> list of byte arrays; `runs` times, equal bits every time"""
    first = launch()
    for _ in range(runs - 1):
        again = launch()
        assert len(first) == len(again) and all(np.array_equal(a, b) for a, b in zip(first, again)), \
            "two launches, different bits"
    return first


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8),
                                                                       b.reshape(-1).view(np.uint8))


@functools.lru_cache(maxsize=None)
def band_operands(bands):
    """scale [bands] float32 (no powers of two: the division must round), shadow ratio [bands] float32"""
    rng = np.random.default_rng([17, bands])
    scale = (rng.random(bands) * 3000 + 7).astype(np.float32)
    ratio = (1 + rng.random(bands) * 4).astype(np.float32)
    return scale, ratio


def clip_of(v):
    """per band the value at 80 % of the ranks, in the source dtype"""
    h, w, bands = v.view.shape
    return np.ascontiguousarray(np.sort(v.view.reshape(h * w, bands), axis=0)[int(0.8 * (h * w - 1))])


def offset_of(v, above):
    """the band minima plus `above`: some samples lie below the offset, so the integer subtraction wraps"""
    return np.ascontiguousarray(v.view.min(axis=(0, 1)) + v.view.dtype.type(above))


# ----------------------------------------------------------------------------------------------------- extrema
def extrema_ref(view, clip, sub):
    v = view if clip is None else np.minimum(view, clip)
    v = v if sub is None else v - sub  # the source dtype's own subtraction
    assert v.dtype == view.dtype
    return v.min(axis=(0, 1)), v.max(axis=(0, 1))


def slice_counts(h, w):
    """1, 3, the number of pixel tiles and 5 more (for either choice of the tile axis), 1024"""
    tiles = {h * -(-w // TILE), w * -(-h // TILE)}
    return sorted({1, 3, 1024} | tiles | {t + 5 for t in tiles})


def run_extrema(be, v, runs=1):
    dtype = v.view.dtype
    item = dtype.itemsize
    src, geom = source(be, v)
    h, w, bands = v.view.shape
    clip, sub = clip_of(v), offset_of(v, 3)
    clip_d, sub_d = up(be, clip), up(be, sub)
    for use_clip in (False, True):
        for use_sub in (False, True):
            want = extrema_ref(v.view, clip if use_clip else None, sub if use_sub else None)
            for ws_slices in slice_counts(h, w):
                def launch():
                    g = Guarded(be, 2 * bands * item, 2 * ws_slices * bands * item)
                    be.call("scene_extrema", src, OUT_DTYPES[dtype], *geom, Ref(clip_d) if use_clip else None,
                            Ref(sub_d) if use_sub else None, g.ref(0), g.ref(0, bands * item), g.ref(1), ws_slices)
                    return g.fetch(0)
                got = issue(launch, runs)[0].view(dtype)
                assert same_bits(got[:bands], want[0]) and same_bits(got[bands:], want[1]), \
                    (v, use_clip, use_sub, ws_slices)


# ----------------------------------------------------------------------------------------------------- rank select
def rank_pairs(n):
    mid, p95 = (n - 1) // 2, int(0.95 * (n - 1))
    return sorted({(0, 0), (n - 1, n - 1), (0, n - 1), (mid, min(mid + 1, n - 1)), (p95, min(p95 + 1, n - 1))})


def run_rank_select(be, v, runs=1):
    assert v.view.dtype == np.uint16
    src, geom = source(be, v)
    h, w, bands = v.view.shape
    srt = np.sort(v.view.reshape(h * w, bands), axis=0)
    for lo, hi in rank_pairs(h * w):
        def launch():
            g = Guarded(be, 4 * bands, bands * SCENE_RANK_WS_WORDS * 4)  # the workspace arrives dirty
            be.call("scene_rank_select_u16", src, *geom, lo, hi, g.ref(0), g.ref(0, 2 * bands), g.ref(1))
            return g.fetch(0)
        got = issue(launch, runs)[0].view(np.uint16)
        assert same_bits(got[:bands], srt[lo]) and same_bits(got[bands:], srt[hi]), (v, lo, hi)


# ----------------------------------------------------------------------------------------------------- prepare
BIG_OUTPUT = 1 << 22  # floats: above it a pad runs with everything on and with everything off only


def pads_of(h, w):
    """0, 1, 5 and one pad above twice the smaller extent: the reflection goes round the scene more than once"""
    return sorted({0, 1, 5, 2 * min(h, w) + 1})


_REFS = {}  # (dtype, the view's key, pad, switches) -> reference; the six stored orders of one scene share theirs


def prepare_ref(v, pad, use_clip, use_lo, use_scale):
    k = (v.view.dtype.str, v.key, pad, use_clip, use_lo, use_scale)
    if k not in _REFS:
        if len(_REFS) >= 40:
            _REFS.pop(next(iter(_REFS)))
        x = v.view if not use_clip else np.minimum(v.view, clip_of(v))
        x = x if not use_lo else x - offset_of(v, 2)  # the source dtype's own subtraction
        assert x.dtype == v.view.dtype
        x = np.pad(x, ((pad, pad), (pad, pad), (0, 0)), mode="symmetric").astype(np.float32)
        _REFS[k] = x / band_operands(v.view.shape[2])[0] if use_scale else x
    return _REFS[k]


def run_prepare(be, v, runs=1, pads=None):
    dtype = v.view.dtype
    src, geom = source(be, v)
    h, w, bands = v.view.shape
    clip_d, lo_d = up(be, clip_of(v)), up(be, offset_of(v, 2))
    scale_d = be.upload(band_operands(bands)[0])
    for pad in pads_of(h, w) if pads is None else pads:
        count = (h + 2 * pad) * (w + 2 * pad) * bands
        configs = ((1, 1, 1), (0, 0, 0)) + (((1, 0, 0), (0, 1, 1)) if count <= BIG_OUTPUT else ())
        for use_clip, use_lo, use_scale in configs:
            def launch():
                g = Guarded(be, count * 4)
                be.call("scene_prepare_f32", src, OUT_DTYPES[dtype], *geom, pad, Ref(clip_d) if use_clip else None,
                        Ref(lo_d) if use_lo else None, Ref(scale_d) if use_scale else None, g.ref(0))
                return g.fetch(0)
            got = issue(launch, runs)[0].view(np.float32)
            want = prepare_ref(v, pad, use_clip, use_lo, use_scale)
            assert same_bits(got.reshape(want.shape), want), (v, pad, use_clip, use_lo, use_scale)


# ----------------------------------------------------------------------------------------------------- correction
def run_shadow_correct(be, v, runs=1):
    from tests.test_components_emu import numpy_correction
    dtype = v.view.dtype
    src, geom = source(be, v)
    h, w, bands = v.view.shape
    smap = (np.random.default_rng([19, h, w]).random((h, w)) < 0.4).astype(np.uint8)
    ratio = band_operands(bands)[1]
    map_d, r_d = be.upload(smap), be.upload(ratio - np.float32(1))

    def launch():
        g = Guarded(be, h * w * bands * 4)
        be.call("shadow_correct_f32", src, OUT_DTYPES[dtype], *geom, Ref(map_d), Ref(r_d), g.ref(0))
        return g.fetch(0)
    got = issue(launch, runs)[0].view(np.float32).reshape(h, w, bands)
    assert same_bits(got, numpy_correction(v.view, smap, ratio)), v


# ----------------------------------------------------------------------------------------------------- masked sums
MASKED_SHAPE = (FULL[0] + 10, FULL[1] + 10, FULL[2])  # the full scene prepared with pad 5: contiguous by contract


def run_masked_sums(be, runs=1):
    hp, wp, bands = MASKED_SHAPE
    n_pix = hp * wp
    rng = np.random.default_rng(23)
    scene32 = ((rng.random(MASKED_SHAPE) - 0.2) * 3).astype(np.float32)
    smap = (rng.random((hp, wp)) < 0.3).astype(np.uint8)
    scene_d, map_d = be.upload(scene32), be.upload(smap)
    on = smap != 0
    s64 = scene32.astype(np.float64)
    by_slicing = {}
    # (1014: the slices 1024 leaves non-empty -- two counts, one slicing)
    for ws_slices in slice_counts(hp, wp) + [-(-n_pix // -(-n_pix // 1024))]:
        def launch():
            g = Guarded(be, (2 * bands + 2) * 8, ws_slices * 2 * (bands + 1) * 8)
            be.call("scene_masked_sums", Ref(scene_d), Ref(map_d), hp, wp, bands, g.ref(0), g.ref(0, 2 * bands * 8),
                    g.ref(1), ws_slices)
            return g.fetch(0)
        raw = issue(launch, runs)[0]
        sums, counts = raw[:2 * bands * 8].view(np.float64).reshape(2, bands), raw[2 * bands * 8:].view(np.int64)
        assert counts.tolist() == [int(on.sum()), int((~on).sum())], ws_slices
        for k, mask in enumerate((on, ~on)):
            exact, mag = s64[mask].sum(axis=0), np.abs(s64[mask]).sum(axis=0)
            # fp64 sums of n < 2^24 float32 values: |error| <= n * 2^-53 * sum|x| in any order (both sides)
            assert np.all(np.abs(sums[k] - exact) <= 2 * mask.sum() * 2.0 ** -53 * mag), ws_slices
        by_slicing.setdefault(-(-n_pix // ws_slices), []).append((ws_slices, raw))
    shared = [runs_ for runs_ in by_slicing.values() if len(runs_) > 1]
    assert shared, "no two slice counts with one slicing"
    for group in shared:
        assert all(np.array_equal(raw, group[0][1]) for _, raw in group), [n for n, _ in group]
