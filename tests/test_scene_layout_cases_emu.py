"""CPU: the cases, references and runners of tests/scene_layout_cases.py on the NumPy twin of the scene launches, so that
they are checked where there is no GPU; then on a second twin that follows csrc/scene.hip's addressing step by step
(fast / other pixel axis, reflected source index, output pitch), first as it is and then with one layout defect planted
at a time -- each defect must be rejected by at least one case.  And device_scene.resident_view on the same views: the
six windowed orders are uploaded in place, a negative or a zero stride is copied."""
import numpy as np
import pytest

import tests.emu_components  # noqa: F401 -- registers the launches on EmuBackend
from hypelcnn_amd.common.device_scene import resident_view
from tests import scene_layout_cases as L
from tests.emu_backend import EmuBackend
from tests.emu_scene import DTYPE_OF, _clip_sub, _typed


# ----------------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: np.dtype(d).name)
def test_extrema(dtype):
    be = EmuBackend()
    for v in L.views(dtype):
        L.run_extrema(be, v)


def test_rank_select():
    be = EmuBackend()
    for v in L.views(np.uint16):
        L.run_rank_select(be, v)


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: np.dtype(d).name)
def test_prepare(dtype):
    be = EmuBackend()
    for v in L.views(dtype):
        L.run_prepare(be, v)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_shadow_correct(dtype):
    be = EmuBackend()
    for v in L.views(dtype):
        L.run_shadow_correct(be, v)


def test_masked_sums():
    L.run_masked_sums(EmuBackend(), runs=2)


def test_case_table():
    table = L.coverage()
    assert {k[:2] for k in table if k[2] == ""} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {k[2] for k in table} == {"", "h", "w", "b", "hw", "hb", "wb", "hwb"}
    for dtype in L.DTYPES:
        lo, hi = L.limits(dtype)
        for v in L.views(dtype):
            assert lo < v.view.min() and v.view.max() < hi and np.isfinite(v.view.astype(np.float64)).all()
        for v in L.window_views(dtype):
            assert v.offset % 2 == 1 and set(np.unique(v.root[:v.offset])) <= {lo, hi}
    assert L.pads_of(*L.FULL[:2])[-1] > 2 * L.FULL[0] and L.rank_pairs(1) == [(0, 0)]


# ----------------------------------------------------------------------------------------------------- planted defects
DEFECTS = ("swapped_pixel_strides", "offset_ignored", "reflect_mode", "unit_extent_stride", "row_pitch", "gap_sample")


def _reflect(i, n, defect):
    if defect == "reflect_mode":  # numpy.pad(mode="reflect"): the edge is not repeated, period 2n - 2
        if n == 1:
            return np.zeros_like(i)
        m = i % (2 * n - 2)
        return np.where(m < n, m, 2 * n - 2 - m)
    m = i % (2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


class AddressingTwin(EmuBackend):
    """The strided launches with the kernels' own addressing: make_geom's two decisions, one gather of the padded tile
    walk [other][fast][band] through element indices, the output scattered through (y * wp + x) * bands + b.  Indices
    wrap at the buffers' ends (a defect must give wrong values here, not a fault).  `defect`: one of DEFECTS."""

    def __init__(self, defect=None):
        super().__init__()
        self.defect = defect

    def _walk(self, src, dtype, h, w, bands, sy, sx, sb, pad):
        """-> (samples [other + 2 pad][fast + 2 pad][bands], y_fast of the walk, y_fast of the output addressing)"""
        far = 2 ** 63 - 1
        ey, ex = (far if h == 1 else sy), (far if w == 1 else sx)
        y_fast = ey < ex
        # the defect: a stride of 0 given for an axis of extent 1 decides the tile axis, the output side knows better
        walk_y = sy < sx if self.defect == "unit_extent_stride" else y_fast
        ext_f, ext_o = (h, w) if walk_y else (w, h)
        sf, so = (sy, sx) if walk_y else (sx, sy)
        if self.defect == "swapped_pixel_strides" and walk_y:
            sf, so = so, sf
        raw = src.t.numpy().reshape(-1).view(np.uint8)
        item = np.dtype(dtype).itemsize
        flat = raw[:raw.size // item * item].view(dtype)
        first = 0 if self.defect == "offset_ignored" else src.off * src.t.element_size() // item
        f = _reflect(np.arange(ext_f + 2 * pad) - pad, ext_f, self.defect)
        o = _reflect(np.arange(ext_o + 2 * pad) - pad, ext_o, self.defect)
        idx = first + o[:, None, None] * so + f[None, :, None] * sf + np.arange(bands)[None, None, :] * sb
        if self.defect == "gap_sample":
            idx[-1, -1, -1] += 1
        return flat.take(idx, mode="wrap"), walk_y, y_fast

    def _logical(self, src, dtype, h, w, bands, sy, sx, sb):
        vals, walk_y, _ = self._walk(src, dtype, h, w, bands, sy, sx, sb, 0)
        return vals.transpose(1, 0, 2) if walk_y else vals

    def k_scene_extrema(self, src, dtype, h, w, bands, sy, sx, sb, clip, sub, out_min, out_max, ws, ws_slices):
        dt = DTYPE_OF[dtype]
        v = _clip_sub(self._logical(src, dt, h, w, bands, sy, sx, sb), dt, bands, clip, sub)
        _typed(out_min, dt, bands)[:] = v.min(axis=(0, 1))
        _typed(out_max, dt, bands)[:] = v.max(axis=(0, 1))

    def k_scene_rank_select_u16(self, src, h, w, bands, sy, sx, sb, rank_lo, rank_hi, out_lo, out_hi, ws):
        v = np.sort(self._logical(src, np.uint16, h, w, bands, sy, sx, sb).reshape(h * w, bands), axis=0)
        _typed(out_lo, np.uint16, bands)[:] = v[rank_lo]
        _typed(out_hi, np.uint16, bands)[:] = v[rank_hi]

    def k_scene_prepare_f32(self, src, dtype, h, w, bands, sy, sx, sb, pad, clip, lo, scale, out):
        dt = DTYPE_OF[dtype]
        vals, _, y_fast = self._walk(src, dt, h, w, bands, sy, sx, sb, pad)
        vals = _clip_sub(vals, dt, bands, clip, lo).astype(np.float32)
        if scale is not None:
            vals = vals / _typed(scale, np.float32, bands)
        oth_pad, ext_pad = vals.shape[:2]
        wp = oth_pad if y_fast else ext_pad
        if self.defect == "row_pitch":
            wp = ext_pad if y_fast else oth_pad
        o, f = np.arange(oth_pad)[:, None, None], np.arange(ext_pad)[None, :, None]
        y, x = (f, o) if y_fast else (o, f)
        dst = _typed(out, np.float32, (h + 2 * pad) * (w + 2 * pad) * bands)
        np.put(dst, (y * wp + x) * bands + np.arange(bands)[None, None, :], vals, mode="wrap")

    def k_shadow_correct_f32(self, src, dtype, h, w, bands, sy, sx, sb, map_, r_minus_1, out):
        c = self._logical(src, DTYPE_OF[dtype], h, w, bands, sy, sx, sb).astype(np.float32)
        m = (_typed(map_, np.uint8, h * w).reshape(h, w, 1) != 0).astype(np.float32)
        _typed(out, np.float32, h * w * bands)[:] = (c + c * (m * _typed(r_minus_1, np.float32, bands))).reshape(-1)


def probes(be, dtype):
    """every runner on every view of one dtype, the small views first; FULL's largest pad left to test_prepare"""
    ordered = [v for v in L.views(dtype) if v.view.shape != L.FULL] + list(L.window_views(dtype))
    for v in ordered:
        yield "prepare", v, lambda v=v: L.run_prepare(be, v, pads=[p for p in L.pads_of(*v.view.shape[:2]) if p < 100])
        yield "extrema", v, lambda v=v: L.run_extrema(be, v)
        if dtype == np.uint16:
            yield "rank_select", v, lambda v=v: L.run_rank_select(be, v)
        yield "shadow_correct", v, lambda v=v: L.run_shadow_correct(be, v)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_addressing_twin_passes_every_case(dtype):
    for _, _, run in probes(AddressingTwin(), dtype):
        run()


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_is_rejected(defect):
    rejected = []
    for launch, v, run in probes(AddressingTwin(defect), np.uint16):
        try:
            run()
        except AssertionError:
            rejected.append((launch, v.name))
            if len({name for name, _ in rejected}) > 1 or len(rejected) >= 8:
                break
    print(f"{defect}: rejected by {rejected}")
    assert rejected, f"no case notices {defect}"


def test_gap_sample_moves_every_launch():
    """one sample from a gap: each of the four strided launches rejects it on the full scene, in every stored order"""
    be = AddressingTwin("gap_sample")
    for v in L.window_views(np.uint16):
        for run in (lambda: L.run_extrema(be, v), lambda: L.run_rank_select(be, v),
                    lambda: L.run_prepare(be, v, pads=[0]), lambda: L.run_shadow_correct(be, v)):
            with pytest.raises(AssertionError):
                run()


# ----------------------------------------------------------------------------------------------------- resident_view
@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: np.dtype(d).name)
def test_resident_view_reads_the_six_orders_in_place(dtype):
    for shape in L.SHAPES:
        for v in L.window_views(dtype, shape):
            root, offset, strides = resident_view(v.view, dtype)
            assert root is v.root and offset == v.offset and strides == v.strides, v


def test_resident_view_copies_what_the_launches_cannot_address():
    full = L.window_views(np.uint16)[3]
    cases = [full.view[::-1], full.view[:, ::-1], full.view[:, :, ::-1], np.broadcast_to(full.view[:1], L.FULL)]
    cases += [v.view for v in L.strided_views(np.uint16)[2:]]
    for a in cases:
        root, offset, strides = resident_view(a, np.uint16)
        assert not np.shares_memory(root, a) and root.flags.c_contiguous and offset == 0, a.strides
        assert np.array_equal(root, a) and min(strides) > 0
        view = np.lib.stride_tricks.as_strided(root.reshape(-1), a.shape, [s * 2 for s in strides])
        assert np.array_equal(view, a)
