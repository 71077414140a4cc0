"""CPU: the template-matching launches on their NumPy emulation (tests/emu_match.py) against the float64 reference of
tests/match_cases.py -- bit for bit on the integer-valued cases, within the stated bounds on the uniform ones -- the
wrapper's refusals, and utilities/lidar_matcher end to end on two synthetic scenes.  The helpers here also drive the
real launches in tests/test_gpu_match.py."""
import json

import numpy as np
import pytest
import torch

import tests.emu_match  # noqa: F401 -- registers the launches on EmuBackend
import tests.emu_scene  # noqa: F401 -- hypel_scene_extrema, which render_u8 takes the maximum from
from hypelcnn_amd.backend import MATCH_BLOCK_COLS, MATCH_COL_CHUNK, MATCH_ROW_CHUNK, MATCH_TILE, Ref
from hypelcnn_amd.common import device_match as dm
from hypelcnn_amd.common.tiff_io import imread
from tests import match_cases as M
from tests.emu_backend import EmuBackend

GUARD = 8  # sentinel elements past the end of every output buffer
F32_SENTINEL = np.array([0x7fc0beef], np.uint32).view(np.float32)[0]  # a NaN with a payload
F64_SENTINEL = np.array([0x7ff8dead0000beef], np.uint64).view(np.float64)[0]
ALL_CASES = [(name, kind) for name in M.CASES for kind in M.KINDS]


SENTINELS = {np.float32: F32_SENTINEL, np.float64: F64_SENTINEL, np.int64: np.int64(0x5a5a5a5a5a5a5a5a)}


def guarded(be, n, dtype):
    return be.upload(np.full(n + GUARD, SENTINELS[dtype], dtype))


def split_guard(t, n, dtype):
    """-> the first n elements; asserts that the sentinels behind them kept their bits"""
    a = t.cpu().numpy()
    assert a.dtype == dtype and a.size == n + GUARD
    assert np.array_equal(bits(a[n:]), bits(np.full(GUARD, SENTINELS[dtype], dtype)))
    return a[:n].copy()


def run_launches(be, case, splits=1, score_map=True):
    """The four launches on guarded buffers -> dict of host arrays: num, energy, e_t, r32 (None without score_map),
    score, index.  Without a score map, a buffer of NaN bits stands by and must stay as it is."""
    img = dm._Band(be, case.image, case.image_scale, "image")
    tpl = dm._Band(be, case.template, case.template_scale, "template")
    n = case.hout * case.wout
    num, energy, e_t = guarded(be, n, np.float32), guarded(be, n, np.float64), guarded(be, 1, np.float64)
    ws_rows, ws_tpl = guarded(be, img.h * case.wout, np.float64), guarded(be, tpl.h, np.float64)
    partials = guarded(be, splits * n, np.float32) if splits > 1 else None
    scores, record = guarded(be, n, np.float32), guarded(be, 2, np.int64)
    be.call("match_ccorr_f32", img.ref, *img.geometry(), tpl.ref, *tpl.geometry(), Ref(num),
            None if partials is None else Ref(partials), splits)
    be.call("match_window_energy_f64", img.ref, *img.geometry(), tpl.H, tpl.W, Ref(energy), Ref(ws_rows))
    be.call("match_window_energy_f64", tpl.ref, *tpl.geometry(), tpl.H, tpl.W, Ref(e_t), Ref(ws_tpl))
    be.call("match_best_f32", Ref(num), Ref(energy), Ref(e_t), case.hout, case.wout,
            Ref(scores) if score_map else None, Ref(record))
    be.synchronize()
    out = {"num": split_guard(num, n, np.float32).reshape(case.hout, case.wout),
           "energy": split_guard(energy, n, np.float64).reshape(case.hout, case.wout),
           "e_t": float(split_guard(e_t, 1, np.float64)[0])}
    split_guard(ws_rows, img.h * case.wout, np.float64)
    split_guard(ws_tpl, tpl.h, np.float64)
    if partials is not None:
        split_guard(partials, splits * n, np.float32)
    rec = split_guard(record, 2, np.int64)
    out["score"], out["index"] = rec.view(np.float32)[0], int(rec[1])
    assert rec.view(np.uint32)[1] == 0
    if score_map:
        out["r32"] = split_guard(scores, n, np.float32).reshape(case.hout, case.wout)
    else:
        untouched = scores.cpu().numpy().view(np.uint32)
        assert np.array_equal(untouched, np.full(n + GUARD, F32_SENTINEL.view(np.uint32), np.uint32))
        out["r32"] = None
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_against_reference(case, got):
    """Prints every figure before it asserts.  int: everything bit for bit.  uniform: the bounds of match_cases."""
    if case.kind == "int":
        assert np.array_equal(bits(got["num"]), bits(case.num.astype(np.float32)))
        assert np.array_equal(bits(got["energy"]), bits(case.energy)) and got["e_t"] == case.e_t
        if got["r32"] is not None:
            assert np.array_equal(bits(got["r32"]), bits(case.r32))
        assert got["index"] == case.index
        assert bits(np.float32(got["score"])) == bits(case.r32.reshape(-1)[case.index])
        return
    num_err = np.abs(got["num"].astype(np.float64) - case.num)
    energy_err = np.abs(got["energy"] - case.energy)
    print(f"{case.name}: num err / bound max {np.max(num_err / np.maximum(case.num_bound, 1e-300)):.3g}, energy err "
          f"{energy_err.max():.3g} (bound {case.energy_bound:.3g}), e_t err {abs(got['e_t'] - case.e_t):.3g}")
    assert np.all(num_err <= case.num_bound)
    assert np.all(energy_err <= case.energy_bound)
    assert abs(got["e_t"] - case.e_t) <= 4 * case.ht * case.wt * M.U53 * case.e_t
    if got["r32"] is not None:
        r_err = np.abs(got["r32"].astype(np.float64) - case.r)
        print(f"{case.name}: R err max {r_err.max():.3g} (bound {case.r_bound:.3g})")
        assert np.all(r_err <= case.r_bound)
    assert case.clear_winner(), "the seed of this case does not give the reference a clear winner"
    assert got["index"] == case.index
    assert abs(float(got["score"]) - case.r.reshape(-1)[case.index]) <= case.r_bound


def pick_splits(case):
    """1 for a template of one (column chunk, row chunk) pair; else a number the pairs do not divide evenly into"""
    units = -(-case.wt // MATCH_COL_CHUNK) * -(-(MATCH_TILE - 1 + case.ht) // MATCH_ROW_CHUNK)
    return 1 if units == 1 else 3 if units % 3 else 5


# ----------------------------------------------------------------------------- the cases themselves
def test_case_shapes_cover_the_launch_geometry():
    c = M.case("chunks_plus_one", "int")
    assert (c.ht, c.wt) == (MATCH_ROW_CHUNK + 1, MATCH_COL_CHUNK + 1)
    assert (c.hout, c.wout) == (2 * MATCH_TILE + 4, 2 * MATCH_TILE + 10) and c.wout < MATCH_BLOCK_COLS
    assert (M.case("whole_image_7x9", "int").hout, M.case("whole_image_7x9", "int").wout) == (1, 1)
    assert M.case("full_height", "int").hout == 1 and M.case("full_width", "int").wout == 1
    s = M.case("scales_5_2", "int")
    assert (s.H, s.W, s.ht, s.wt) == (65, 85, 18, 22)
    assert M.case("strided_bands", "int").image.strides == (24 * 5 * 4, 5 * 4)
    z = M.case("zero_block", "int")
    assert (z.r32 == 0).sum() >= 7 * 8 and z.r32.max() > 0
    a = M.case("all_zero_image", "int")
    assert a.index == 0 and not a.r32.any()
    t = M.case("ties_periodic", "int")
    flat = t.r32.reshape(-1)
    assert (bits(flat) == bits(flat[t.index:t.index + 1])[0]).sum() >= 4 and t.index < 3 * t.wout  # several equal maxima


@pytest.mark.parametrize("name", list(M.CASES))
def test_uniform_cases_have_a_clear_winner(name):
    assert M.case(name, "uniform").clear_winner()


@pytest.mark.parametrize("name,kind", ALL_CASES)
def test_launches_against_the_reference(name, kind):
    case = M.case(name, kind)
    be = EmuBackend()
    check_against_reference(case, run_launches(be, case, splits=pick_splits(case)))
    check_against_reference(case, run_launches(be, case, splits=1, score_map=False))


@pytest.mark.parametrize("name,kind", ALL_CASES)
def test_match_template_wrapper(name, kind):
    case = M.case(name, kind)
    found = dm.match_template(EmuBackend(), case.image, case.template, case.image_scale, case.template_scale,
                              keep_scores=True)
    assert found.shape == (case.hout, case.wout) and found.index == case.index
    y, x = divmod(case.index, case.wout)
    assert found.top_left == (x, y) and found.bottom_right == (x + case.wt, y + case.ht)
    assert found.scores.dtype == torch.float32 and found.scores.numel() == case.hout * case.wout
    assert abs(found.score - case.r.reshape(-1)[case.index]) <= case.r_bound
    assert dm.match_template(EmuBackend(), case.image, case.template, case.image_scale,
                             case.template_scale).scores is None


def test_device_tensors_are_read_through_their_strides():
    case = M.case("strided_bands", "int")
    be = EmuBackend()
    scene = torch.from_numpy(np.ascontiguousarray(case.image.base))  # [h, w, 5]
    found = dm.match_template(be, scene[:, :, 3], torch.from_numpy(case.template.copy()))
    assert found.index == case.index
    band = dm._Band(be, scene[:, :, 3], 1, "image")
    assert (band.sy, band.sx) == (24 * 5, 5) and band.flat.data_ptr() == scene.data_ptr() + 3 * 4  # no copy


def test_choose_splits():
    assert dm.choose_splits(1, 1, 1, 1) == 1
    assert dm.choose_splits(36, 42, 33, 33) == 1  # four chunk pairs: not worth a split
    assert dm.choose_splits(36, 42, 33, 33 * 32) == 4  # 66 pairs: 16 at least per split
    # the contest geometry: 3 x 11 blocks of tiles, 257 x 54 chunk pairs -> 496 splits of 28 pairs
    assert dm.choose_splits(42, 1332, 1704, 8194) == 496
    assert dm.choose_splits(4000, 4000, 1704, 8194) == 2 and dm.choose_splits(8000, 8000, 1704, 8194) == 1
    assert dm.choose_splits(4000, 4000, 1704, 8194) * 16000000 <= dm.MAX_PARTIAL_FLOATS


def test_wrapper_refuses_by_name():
    be = EmuBackend()
    image, template = np.ones((6, 8), np.float32), np.ones((3, 4), np.float32)
    with pytest.raises(NotImplementedError, match="not an integer"):
        dm.match_template(be, image, template, image_scale=2.5)
    with pytest.raises(NotImplementedError, match="below 1"):
        dm.match_template(be, image, template, template_scale=0)
    with pytest.raises(ValueError, match="larger than the enlarged image"):
        dm.match_template(be, image, template, template_scale=3)
    with pytest.raises(ValueError, match="2-D"):
        dm.match_template(be, np.ones((2, 3, 4), np.float32), template)
    with pytest.raises(ValueError, match=r"2\*\*31"):
        dm.match_template(be, np.ones((5, 5), np.float32), template, image_scale=10000)
    with pytest.raises(ValueError, match="splits"):
        dm.match_template(be, image, template, splits=0)


def test_render_is_numpys_expression():
    rng = np.random.default_rng(3)
    scene = rng.random((9, 11, 4)).astype(np.float32)
    band = scene[:, :, 2]
    be = EmuBackend()
    got = dm.render_u8(be, dm._Band(be, band, 3, "image")).numpy().reshape(27, 33)
    big = M.replicate(band, 3)
    assert got.dtype == np.uint8 and np.array_equal(got, (big / np.max(big) * 255).astype("uint8"))
    assert got.max() == 255


# ----------------------------------------------------------------------------- the command line
CLI = ["--image_loader", "SyntheticDataLoader", "--image_path", "grss2013:h=24:w=40",
       "--template_loader", "SyntheticDataLoader", "--template_path", "grss2018:h=14:w=20",
       "--template_crop", "3,2", "--image_scale", "5", "--template_scale", "2"]


def cli_reference():
    """the same bands from the loader, through the reference of match_cases -> (image band, template band, index, r)"""
    from hypelcnn_amd.loader.SyntheticDataLoader import SyntheticDataLoader
    image = SyntheticDataLoader("grss2013:h=24:w=40").load_data(0, True).casi[:, :, 8].astype(np.float32)
    template = SyntheticDataLoader("grss2018:h=14:w=20").load_data(0, True).casi[:, :, 2].astype(np.float32)[:-3, :-2]
    big, tpl = M.replicate(image.astype(np.float64), 5), M.replicate(template.astype(np.float64), 2)
    windows = np.lib.stride_tricks.sliding_window_view(big, tpl.shape)
    r = np.einsum("yxij,ij->yx", windows, tpl) / np.sqrt(np.einsum("yxij,yxij->yx", windows, windows) * (tpl * tpl).sum())
    return image, template, int(np.argmax(r.astype(np.float32).reshape(-1))), r


def check_cli_outputs(result, out_dir, printed):
    image, template, index, r = cli_reference()
    y, x = divmod(index, r.shape[1])
    bound = (22 * 36 + 16) * M.U24
    assert result["top_left"] == [x, y] and result["bottom_right"] == [x + 36, y + 22]
    assert result["top_left_scaled"] == [x / 5, y / 5] and result["bottom_right_scaled"] == [(x + 36) / 5, (y + 22) / 5]
    assert abs(result["score"] - r[y, x]) <= bound
    geometry = result["geometry"]
    assert geometry["image"] == {"loader": "SyntheticDataLoader", "band": 8, "bands": 144, "shape": [24, 40], "scale": 5}
    assert geometry["template"] == {"loader": "SyntheticDataLoader", "band": 2, "bands": 48, "shape": [11, 18],
                                    "scale": 2, "crop": [3, 2]}
    assert geometry["surface"] == [120 - 22 + 1, 200 - 36 + 1]
    assert printed == [f"Top Left ({x}, {y})", "Top Left(scaled) (%f, %f)" % (x / 5, y / 5),
                       f"Bottom Right ({x + 36}, {y + 22})",
                       "Bottom Right(scaled) (%f, %f)" % ((x + 36) / 5, (y + 22) / 5)]
    with open(str(out_dir) + "/lidar_match.json") as f:
        assert json.load(f) == result
    figure = imread(str(out_dir) + "/lidar_match.tif")
    assert figure.dtype == np.uint8 and figure.shape == (120, 200)
    grey = (M.replicate(image, 5) / np.max(image) * 255).astype("uint8")
    frame = figure != grey
    assert np.all(figure[frame] == 255)
    for fy, fx in ((y, x), (y, x + 35), (y + 21, x), (y + 21, x + 35), (y, x + 18), (y + 11, x)):
        assert figure[fy, fx] == 255  # on the rectangle's edge (20 pixels wide, centred on it)
    if y + 11 < 120 and x + 18 < 200:
        assert figure[y + 11, x + 18] == grey[y + 11, x + 18]  # the middle of a 22 x 36 rectangle is not
    return index


def test_lidar_matcher_end_to_end(tmp_path, capsys):
    from hypelcnn_amd.utilities import lidar_matcher
    result = lidar_matcher.main(CLI + ["--output_path", str(tmp_path)], backend=EmuBackend())
    check_cli_outputs(result, tmp_path, capsys.readouterr().out.splitlines())


def test_draw_frame_clips_to_the_raster():
    from hypelcnn_amd.utilities.lidar_matcher import draw_frame
    raster = np.zeros((30, 40), np.uint8)
    draw_frame(raster, (0, 20), (40, 30), 4)
    assert raster[18:22, :].min() == 255 and raster[28:, :].min() == 255 and raster[22:28, 2:38].max() == 0
    assert raster[18:, :2].min() == 255 and raster[18:, 38:].min() == 255 and raster[:18].max() == 0


def test_lidar_matcher_refusals(tmp_path):
    from hypelcnn_amd.utilities import lidar_matcher
    be = EmuBackend()

    def run(*changed):
        args = list(CLI)
        for flag, value in zip(changed[::2], changed[1::2]):
            args[args.index(flag) + 1] = value
        return lidar_matcher.main(args + ["--output_path", str(tmp_path)], backend=be)

    with pytest.raises(NotImplementedError, match="2.5.*not an integer"):
        run("--template_scale", "2.5")
    with pytest.raises(ValueError, match="--template_crop 14,2 leaves nothing"):
        run("--template_crop", "14,2")
    with pytest.raises(ValueError, match="larger than the enlarged image"):
        run("--template_scale", "12")
    with pytest.raises(ValueError, match="--image_band 144 is outside 0..143"):
        lidar_matcher.main(CLI + ["--image_band", "144", "--output_path", str(tmp_path)], backend=be)
    with pytest.raises(ValueError, match="--template_band -1 is outside 0..47"):
        lidar_matcher.main(CLI + ["--template_band", "-1", "--output_path", str(tmp_path)], backend=be)
    assert not (tmp_path / "lidar_match.json").exists()


def test_lidar_matcher_needs_a_device(tmp_path, monkeypatch):
    from hypelcnn_amd.backend import HypelError
    from hypelcnn_amd.utilities import lidar_matcher
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(HypelError, match="no CPU fallback"):
        lidar_matcher.main(CLI + ["--output_path", str(tmp_path)])
