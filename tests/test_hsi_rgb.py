"""sRGB rendering on the CPU: the known answers that pin the typed CIE 1931 table, band selection against the
reference's literal loop, the observer names, the weight table of hypel_hsi_to_srgb, and gan_infer_image_for_shadow
--rgb end to end on the emulation (tests/rgb_cases.py RgbEmu) against the float64 oracle."""
import os

import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import RGB_F32, RGB_U8
from hypelcnn_amd.common import hsi_rgb_converter as HR
from hypelcnn_amd.common import tiff_io
from hypelcnn_amd.gan import gan_infer_image_for_shadow as GI
from hypelcnn_amd.loader.SyntheticDataLoader import SyntheticDataLoader
from tests import rgb_cases as RC
from tests.test_gan_inference import SCENE, ScriptedGenerator, _trained_checkpoint

SENSORS = {"grss2013": np.linspace(380, 1050, 144), "grss2018": np.linspace(380, 1050, 48),
           "gulfport": np.linspace(405, 1005, 64), "avon": np.linspace(400, 2500, 360)}


# ----------------------------------------------------------------------------- the typed table
@pytest.mark.parametrize("table", [HR.CIE1931_2, RC.CMF], ids=["package", "oracle"])
def test_column_sums_of_the_observer(table):
    assert table.shape == (31, 3)
    sums = table.sum(axis=0)
    assert np.allclose(sums, [10.666589, 10.681488, 10.650400], rtol=0, atol=5e-7), sums
    assert np.abs(sums / sums.mean() - 1).max() < 3e-3  # an equal-energy white


def test_package_and_oracle_tables_are_the_same_numbers():
    assert np.array_equal(HR.CIE1931_2, RC.CMF)


def test_flat_white_and_black_oracle():
    bm = np.linspace(400, 700, 31)
    assert (RC.oracle_rgb(bm, np.ones((1, 31))) * 255).astype(np.uint8).tolist() == [[255, 249, 244]]
    assert (RC.oracle_rgb(bm, np.zeros((1, 31))) * 255).astype(np.uint8).tolist() == [[0, 0, 0]]


@pytest.mark.parametrize("bands", [8, 31, 144])
def test_flat_white_and_black_through_the_package(bands):
    bm = RC.measurements(bands)
    scene = np.stack([np.ones((2, bands), np.float32), np.zeros((2, bands), np.float32)])
    rgb = HR.get_rgb_from_hsi(bm, scene, backend=RC.RgbEmu())
    assert rgb.shape == (2, 2, 3) and rgb.dtype == np.float32
    assert (rgb * 255).astype(np.uint8).tolist() == [[[255, 249, 244]] * 2, [[0, 0, 0]] * 2]
    as_tensor = HR.get_rgb_from_hsi(bm, torch.from_numpy(scene), backend=RC.RgbEmu())
    assert isinstance(as_tensor, torch.Tensor) and np.array_equal(as_tensor.numpy(), rgb)
    u16 = (scene.reshape(4, bands) * 60000 + 100).astype(np.uint16)
    got = HR.render_raster_rgb(RC.RgbEmu(), torch.from_numpy(u16.reshape(-1).copy()), np.uint16, 2, 2, bands, bm,
                               np.uint16(100), np.uint16(60000))
    assert got.dtype == np.uint8 and got.tolist() == [[[255, 249, 244]] * 2, [[0, 0, 0]] * 2]


# ----------------------------------------------------------------------------- band selection
@pytest.mark.parametrize("name", list(SENSORS))
def test_selection_on_the_sensors(name):
    bm = SENSORS[name]
    sel = HR.select_visual_bands(bm)
    assert sel == RC.oracle_select(bm) and len(sel) == 31
    assert all(isinstance(i, int) for i in sel)
    if name in ("grss2013", "avon"):
        assert len(set(sel)) == 31  # finer than 10 nm from 400 nm on: every wavelength has a band of its own
    if name == "gulfport":
        assert sel[:3] == [0, 0, 2]  # 405 nm is nearest to 400, and ties with 415 nm for 410: the first index wins
    nearest = np.abs(np.round(bm)[sel] - np.arange(400, 701, 10))
    assert nearest.max() <= {"grss2013": 3, "grss2018": 7, "gulfport": 5, "avon": 3}[name]


def test_selection_with_few_bands_gives_duplicates():
    bm = np.linspace(400, 700, 8)
    sel = HR.select_visual_bands(bm)
    assert sel == RC.oracle_select(bm)
    assert sorted(set(sel)) == list(range(8)) and len(sel) == 31
    assert sel == sorted(sel)


def test_selection_above_the_visual_range_is_band_zero():
    bm = np.linspace(900, 1700, 40)
    assert HR.select_visual_bands(bm) == RC.oracle_select(bm) == [0] * 31


def test_selection_tie_goes_to_the_first_index():
    bm = np.array([394.6, 405.4, 414.8, 425.3, 700.0])  # rounds to 395, 405, 415, 425: 400, 410 and 420 are ties
    sel = HR.select_visual_bands(bm)
    assert sel == RC.oracle_select(bm)
    assert sel[:3] == [0, 1, 2] and sel[-1] == 4
    assert HR.select_visual_bands(bm[::-1])[:3] == [3, 2, 1]  # reversed, each tie goes to the other member of the pair


def test_observer_names():
    assert HR.get_cmfs("cie1931_2") is HR.CIE1931_2
    for name in ("cie1964_10", "cie2012_2", "cie2012_10"):
        with pytest.raises(NotImplementedError, match=name):
            HR.get_cmfs(name)
        with pytest.raises(NotImplementedError, match=name):
            HR.render_table(np.linspace(400, 700, 31), 31, cmf_name=name)
    with pytest.raises(AttributeError, match="Wrong cmf name"):
        HR.get_cmfs("cie1931_10")


# ----------------------------------------------------------------------------- the weight table
@pytest.mark.parametrize("bands", [8, 31, 48, 144, 360])
@pytest.mark.parametrize("per_band", [False, True])
def test_weight_table_folds_selection_and_normalisation(bands, per_band):
    rng = np.random.default_rng(bands)
    bm = RC.measurements(bands)
    lo, hi = RC.normalisation(np.uint16, bands, per_band, rng)
    band0, span, table = HR.render_table(bm, bands, hi, lo)
    sel = RC.oracle_select(bm)
    assert table.dtype == np.float64 and table.shape == (span, 4)
    assert band0 % 4 == 0 and band0 <= min(sel) and max(sel) < band0 + span <= bands
    assert (band0 + span) % 4 == 0 or band0 + span == bands
    v = rng.integers(0, 65535, (5, bands)).astype(np.float64)
    xyz = (v[:, band0:band0 + span] - table[:, 0]) @ table[:, 1:]
    r = RC.normalise(v, lo, hi)
    want = (r[:, sel, None] * RC.CMF).sum(axis=1) / RC.CMF[:, 1].sum()
    assert np.abs(xyz - want).max() < 1e-14
    unpicked = np.setdiff1d(np.arange(band0, band0 + span), sel) - band0
    assert not table[unpicked].any()


def test_levels_are_the_first_values_the_float64_expression_renders_as_k():
    lv = HR.srgb_levels()
    assert lv.shape == (256,) and lv.dtype == np.float64 and lv[0] == -np.inf and (np.diff(lv) > 0).all()
    k = np.arange(1, 256)
    at, below = lv[1:], np.nextafter(lv[1:], -np.inf)
    assert (RC.oracle_rgb_of_linear(at) * 255).astype(np.uint8).tolist() == k.tolist()
    assert (RC.oracle_rgb_of_linear(below) * 255).astype(np.uint8).tolist() == (k - 1).tolist()
    assert abs(lv[255] - 1.0) < 1e-15 and abs(lv[1] - 1 / 255 / 12.92) < 1e-18


def test_measurements_longer_than_the_raster_are_refused():
    with pytest.raises(ValueError, match="bands"):
        HR.render_table(np.linspace(400, 700, 31), 16)


# ----------------------------------------------------------------------------- emulation against the oracle
@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.int16, np.uint8])
@pytest.mark.parametrize("bands,pad,per_band", [(8, 0, True), (31, 3, False), (144, 4, True)])
def test_emulated_launch_against_the_oracle(dtype, bands, pad, per_band):
    from hypelcnn_amd.backend import Ref
    rng = np.random.default_rng(bands + np.dtype(dtype).itemsize)
    h, w = 7, 9
    bm = RC.measurements(bands)
    lo, hi = RC.normalisation(dtype, bands, per_band, rng)
    raster = RC.edge_raster(h, w, bands, bands + pad, dtype, lo, hi, rng)
    be = RC.RgbEmu()
    dev = be.upload(raster)
    want = RC.oracle_rgb(bm, RC.normalise(raster[:, :bands], lo, hi))
    out = HR.launch_render(be, Ref(dev), dtype, bands + pad, h * w, bands, bm, hi, lo, RGB_U8)
    RC.check_u8(out.numpy().reshape(h * w, 3), (want * 255).astype(np.uint8))
    out = HR.launch_render(be, Ref(dev), dtype, bands + pad, h * w, bands, bm, hi, lo, RGB_F32)
    assert np.abs(out.numpy().reshape(h * w, 3) - want).max() < 2e-5


# ----------------------------------------------------------------------------- convert_scene and the CLI
def test_convert_scene_renders_what_it_returns():
    loader = SyntheticDataLoader("gulfport:h=9:w=11:bands=12:lidar=1:dtype=uint16:lo=400:hi=700")
    ds = loader.load_data(0, True)
    smap, _ = loader.load_shadow_map(0, ds)
    plain = GI.convert_scene(ds, smap, "shadow", False, ScriptedGenerator(12), RC.RgbEmu(), chunk=7)
    timings = {}
    image, rgb = GI.convert_scene(ds, smap, "shadow", False, ScriptedGenerator(12), RC.RgbEmu(), chunk=7,
                                  timings=timings, rgb_band_measurements=loader.get_band_measurements())
    assert np.array_equal(image, plain) and image.dtype == np.uint16
    assert rgb.dtype == np.uint8 and rgb.shape == (9, 11, 3) and "rgb_s" in timings
    RC.check_u8(rgb, RC.oracle_u8(loader.get_band_measurements(), image, ds.casi_min, ds.casi_max))
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 20  # a picture, not a constant


def test_cli_writes_the_rgb_rendering_under_the_references_name(tmp_path):
    ckpt = _trained_checkpoint(tmp_path, "cycle_gan", steps=4)
    step = ckpt.rsplit("-", 1)[-1][:-4]
    scene = SCENE + ":dtype=uint16"
    loader = SyntheticDataLoader(scene)
    ds = loader.load_data(0, True)
    out = tmp_path / "out"
    names = []
    for mode, conv_all, sfx in (("shadow", "false", ""), ("deshadow", "false", ""), ("none", "true", "_all")):
        img, path = GI.main(["--loader_name", "SyntheticDataLoader", "--path", scene, "--base_log_path", ckpt,
                             "--make_them_shadow", mode, "--convert_all", conv_all, "--rgb", "true",
                             "--output_path", str(out)], backend=RC.RgbEmu(), chunk=50)
        assert os.path.basename(path) == f"shadow_image_{mode}_{step}{sfx}.tif"
        rgb_name = f"shadow_image_rgb_{mode}_{step}_{sfx}.tif"
        names += [os.path.basename(path), rgb_name]
        hsi = tiff_io.imread(path)
        assert np.array_equal(hsi, img)
        rgb = tiff_io.imread(str(out / rgb_name))
        assert rgb.dtype == np.uint8 and rgb.shape == (12, 14, 3)
        RC.check_u8(rgb, RC.oracle_u8(loader.get_band_measurements(), hsi, ds.casi_min, ds.casi_max))
    assert names[1::2] == [f"shadow_image_rgb_shadow_{step}_.tif", f"shadow_image_rgb_deshadow_{step}_.tif",
                           f"shadow_image_rgb_none_{step}__all.tif"]
    assert sorted(os.listdir(out)) == sorted(names)


def test_cli_without_the_flag_writes_one_file(tmp_path, capsys):
    ckpt = _trained_checkpoint(tmp_path, "cycle_gan", steps=2)
    step = ckpt.rsplit("-", 1)[-1][:-4]
    out = tmp_path / "out"
    for extra in ([], ["--rgb", "false"]):
        GI.main(["--loader_name", "SyntheticDataLoader", "--path", SCENE + ":dtype=uint16", "--base_log_path", ckpt,
                 "--make_them_shadow", "shadow", "--output_path", str(out)] + extra, backend=RC.RgbEmu(), chunk=50)
        assert os.listdir(out) == [f"shadow_image_shadow_{step}.tif"]
    assert GI.build_parser().parse_known_args([])[0].rgb is False
    assert "RGB rendering skipped" in capsys.readouterr().out
