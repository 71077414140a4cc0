"""-m gpu: hypel_hsi_to_srgb on the MI355X against the float64 oracle of tests/rgb_cases.py, and convert_scene with the
rendering enabled.  Rasters of 7 x 9 and 37 x 53 pixels (no multiple of a wave or a block); every input dtype; 8 (picked
bands repeat), 31, 48, 144 and 360 bands; rows tight, padded by 3 (one band per lane), padded to a multiple of 4 (four
bands per lane, with a tail at 31 bands) and tight behind a two-element offset (misaligned base); scalar and per-band
normalisation; both output modes."""
import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import RGB_F32, RGB_U8, Ref
from hypelcnn_amd.common import hsi_rgb_converter as HR
from hypelcnn_amd.gan import gan_infer_image_for_shadow as GI
from hypelcnn_amd.loader.SyntheticDataLoader import SyntheticDataLoader
from tests import rgb_cases as RC

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.uint16, np.int16, np.uint8]
BANDS = [8, 31, 48, 144, 360]
SIZES = [(7, 9), (37, 53)]
LAYOUTS = ["tight", "pad3", "pad4", "shifted"]
# (row layout, casi_min / casi_max per band): every layout, and both kinds of normalisation on aligned and on
# misaligned rows
SUBCASES = [("tight", False), ("tight", True), ("pad3", True), ("pad4", False), ("shifted", True), ("pad3", False)]


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


def _ld(bands, layout):
    return {"pad3": bands + 3, "pad4": (bands + 3) // 4 * 4 + 4}.get(layout, bands)


@pytest.fixture(scope="module")
def cases():
    """Every raster of this module with its float64 rendering and the float32 chain's distance from it, built once."""
    out = {}
    for dtype in DTYPES:
        for bands in BANDS:
            for h, w in SIZES:
                for layout, per_band in SUBCASES:
                    rng = np.random.default_rng([np.dtype(dtype).num, bands, h, LAYOUTS.index(layout), per_band])
                    bm = RC.measurements(bands)
                    lo, hi = RC.normalisation(dtype, bands, per_band, rng)
                    raster = RC.edge_raster(h, w, bands, _ld(bands, layout), dtype, lo, hi, rng)
                    want = RC.oracle_rgb(bm, RC.normalise(raster[:, :bands], lo, hi))
                    f32 = RC.float32_rgb(bm, RC.normalise(raster[:, :bands], lo, hi, np.float32))
                    out[(np.dtype(dtype), bands, h, layout, per_band)] = (raster, lo, hi, bm, want,
                                                                          float(np.abs(f32 - want).max()))
    return out


def _launch(hip, raster, dtype, layout, bands, h, w, bm, lo, hi, mode):
    shift = 2 if layout == "shifted" else 0
    flat = np.concatenate([np.zeros(shift, raster.dtype), raster.reshape(-1)])
    out = HR.launch_render(hip, Ref(hip.upload(flat), shift), dtype, raster.shape[1], h * w, bands, bm, hi, lo, mode)
    hip.synchronize()
    return out.cpu().numpy().reshape(h * w, 3)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_u8_rendering(hip, cases, dtype, bands, size):
    """No sample further than 1 from (oracle * 255).astype(uint8), at most 0.1 % of a raster's samples different at all
    (tests/rgb_cases.py check_u8, which prints the share).  Observed on an MI355X: 0 on every raster."""
    h, w = size
    for layout, per_band in SUBCASES:
        raster, lo, hi, bm, want, _ = cases[(np.dtype(dtype), bands, h, layout, per_band)]
        got = _launch(hip, raster, dtype, layout, bands, h, w, bm, lo, hi, RGB_U8)
        RC.check_u8(got, (want * 255).astype(np.uint8))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bands", BANDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_f32_rendering(hip, cases, dtype, bands, size):
    """float32 rgb of every raster within 4 x the distance of the float32 NumPy chain from the float64 oracle on that
    same raster; the margin covers the device's exp2 / log2 and another summation order.  The bounds of the 240 rasters
    run from 7.0e-7 to 1.42e-5; observed on an MI355X: 1.4e-07 at most, never above 0.16 of a raster's bound."""
    h, w = size
    for layout, per_band in SUBCASES:
        raster, lo, hi, bm, want, chain = cases[(np.dtype(dtype), bands, h, layout, per_band)]
        got = _launch(hip, raster, dtype, layout, bands, h, w, bm, lo, hi, RGB_F32)
        assert got.dtype == np.float32 and got.min() >= 0.0 and got.max() <= 1.0
        worst, bound = float(np.abs(got - want).max()), 4 * chain
        print(f"\nf32 rendering: largest distance from the oracle {worst:.3e}, bound {bound:.3e}, "
              f"share of the bound {worst / bound:.2f}")
        assert worst <= bound, (layout, per_band, worst, bound)


def test_edge_rows_reach_both_clips_and_both_pieces_of_the_curve(cases):
    """The rasters do contain what the module's docstring promises (checked on the oracle, so that a change of the
    builder cannot quietly drop an edge)."""
    raster, lo, hi, bm, want, _ = cases[(np.dtype(np.uint16), 144, 7, "tight", False)]
    r = RC.normalise(raster[:, :144], lo, hi)
    lin = (r[:, RC.oracle_select(bm), None] * RC.CMF).sum(axis=1) / RC.CMF[:, 1].sum() @ np.linalg.inv(RC.XYZ_FROM_RGB).T
    assert (lin < 0).any() and (lin > 1).any()
    assert ((lin > 0) & (lin < RC.KNEE)).any() and ((lin > RC.KNEE) & (lin < 1.2 * RC.KNEE)).any()
    assert (want == 0).any() and (want == 1).any() and (raster[:, :144] == 65535).all(axis=1).any()
    assert (raster[:, :144] == 0).all(axis=1).any()


def test_non_finite_input_renders_black(hip):
    """Documented, not compared with NumPy: a pixel with a non-finite sample in its span renders as 0; its neighbours
    are untouched."""
    bands, h, w = 48, 3, 5
    bm = RC.measurements(bands)
    rng = np.random.default_rng(3)
    raster = (0.2 + 0.6 * rng.random((h * w, bands))).astype(np.float32)
    clean = _launch(hip, raster, np.float32, "tight", bands, h, w, bm, None, None, RGB_U8)
    sel = RC.oracle_select(bm)
    raster[2, sel[4]], raster[7, sel[20]], raster[11, sel[30]] = np.nan, np.inf, -np.inf
    got = _launch(hip, raster, np.float32, "tight", bands, h, w, bm, None, None, RGB_U8)
    bad = np.zeros(h * w, bool)
    bad[[2, 7, 11]] = True
    assert (got[bad] == 0).all() and np.array_equal(got[~bad], clean[~bad]) and (clean[bad] > 0).all()
    assert (_launch(hip, raster, np.float32, "tight", bands, h, w, bm, None, None, RGB_F32)[bad] == 0).all()


def test_get_rgb_from_hsi_on_numpy_and_device_input(hip):
    bm = RC.measurements(144)
    scene = np.random.default_rng(0).random((7, 9, 144)).astype(np.float32)
    want = RC.oracle_rgb(bm, scene)
    a = HR.get_rgb_from_hsi(bm, scene, backend=hip)
    b = HR.get_rgb_from_hsi(bm, torch.from_numpy(scene).to(hip.device), backend=hip)
    assert isinstance(a, np.ndarray) and a.shape == (7, 9, 3) and a.dtype == np.float32
    assert isinstance(b, torch.Tensor) and b.is_cuda and np.array_equal(b.cpu().numpy(), a)
    bound = 4 * float(np.abs(RC.float32_rgb(bm, scene) - want).max())  # the rule of test_f32_rendering, on this scene
    assert np.abs(a - want).max() <= bound, (np.abs(a - want).max(), bound)


class DeviceScriptedGenerator:
    """tests/test_gan_inference.py ScriptedGenerator with its buffers on the device: g(x) = tanh(1.7 x - 0.4 + 0.01 b),
    returned as rows of stride bands + 3."""

    def __init__(self, bands, device):
        self.bands, self.device, self._in = bands, device, {}

    def input(self, n):
        if n not in self._in:
            self._in[n] = torch.zeros(n * self.bands, device=self.device)
        return self._in[n]

    def __call__(self, n):
        x = self._in[n].reshape(n, self.bands)
        out = torch.zeros(n, self.bands + 3, device=self.device)
        out[:, :self.bands] = torch.tanh(1.7 * x - 0.4 + 0.01 * torch.arange(self.bands, device=self.device))
        return out[:, :self.bands]


@pytest.mark.parametrize("mode,convert_all", [("shadow", False), ("none", True)])
def test_convert_scene_with_the_rendering(hip, mode, convert_all):
    """The synthetic 12 x 14 x 16 uint16 scene: the rendering equals the oracle applied to the returned scene under the
    uint8 rule, and the scene is bit for bit the one of a run without the rendering."""
    loader = SyntheticDataLoader("gulfport:h=12:w=14:bands=16:classes=3:samples=0.6:dtype=uint16")
    ds = loader.load_data(0, True)
    smap, _ = loader.load_shadow_map(0, ds)
    bm = loader.get_band_measurements()
    plain = GI.convert_scene(ds, smap, mode, convert_all, DeviceScriptedGenerator(16, hip.device), hip, chunk=50)
    image, rgb = GI.convert_scene(ds, smap, mode, convert_all, DeviceScriptedGenerator(16, hip.device), hip, chunk=50,
                                  rgb_band_measurements=bm)
    assert image.dtype == np.uint16 and image.shape == (12, 14, 16)
    assert np.array_equal(image, plain)
    assert rgb.dtype == np.uint8 and rgb.shape == (12, 14, 3)
    RC.check_u8(rgb, RC.oracle_u8(bm, image, ds.casi_min, ds.casi_max))
