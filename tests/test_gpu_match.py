"""GPU: the template-matching launches of csrc/match.hip against the float64 reference of tests/match_cases.py -- the
integer-valued cases bit for bit (numerator, window energies, float32 score surface, index), the uniform ones within the
any-order float32 summation bound and the double prefix-sum bound, the location under the asserted clear-winner
precondition -- with sentinels behind every output buffer, with and without column splits and the optional score map,
every launch twice with identical bits; the wrapper on device tensors read through their strides; the figure raster
against NumPy's expression; and utilities/lidar_matcher on the device against the same run on the NumPy emulation."""
import numpy as np
import pytest
import torch

from hypelcnn_amd.common import device_match as dm
from tests import match_cases as M
from tests.test_match_emu import ALL_CASES, CLI, bits, check_against_reference, check_cli_outputs, pick_splits, run_launches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.mark.parametrize("name,kind", ALL_CASES)
def test_launches_against_the_reference(be, name, kind):
    case = M.case(name, kind)
    split = run_launches(be, case, splits=pick_splits(case))
    check_against_reference(case, split)
    plain = run_launches(be, case, splits=1, score_map=False)
    check_against_reference(case, plain)
    again = run_launches(be, case, splits=pick_splits(case))
    for key in ("num", "energy", "r32"):
        assert np.array_equal(bits(again[key]), bits(split[key])), key
    assert (again["e_t"], again["index"]) == (split["e_t"], split["index"])
    assert bits(np.float32(again["score"])) == bits(np.float32(split["score"]))


def test_more_splits_than_column_chunks(be):
    case = M.case("chunks_plus_one", "int")  # four chunk pairs dealt to five splits: the last one adds zeros
    check_against_reference(case, run_launches(be, case, splits=5))


@pytest.mark.parametrize("name,kind", [("strided_bands", "int"), ("strided_bands_scaled", "uniform"),
                                       ("scales_5_2", "uniform"), ("ties_periodic", "int"),
                                       ("transposed_band", "int"), ("transposed_band", "uniform")])
def test_wrapper_on_host_arrays_and_device_tensors(be, name, kind):
    case = M.case(name, kind)
    found = dm.match_template(be, case.image, case.template, case.image_scale, case.template_scale, keep_scores=True)
    assert found.index == case.index and found.shape == (case.hout, case.wout)
    surface = found.scores.cpu().numpy().reshape(found.shape)
    assert np.all(np.abs(surface.astype(np.float64) - case.r) <= case.r_bound)
    # the same bands as views of tensors that are on the device already
    image_d = torch.from_numpy(np.ascontiguousarray(case.image)).to(be.device)
    wide = torch.zeros((case.template.shape[0], case.template.shape[1], 3), device=be.device)
    wide[:, :, 1] = torch.from_numpy(np.ascontiguousarray(case.template)).to(be.device)
    on_device = dm.match_template(be, image_d, wide[:, :, 1], case.image_scale, case.template_scale, keep_scores=True)
    assert on_device.index == found.index and torch.equal(on_device.scores, found.scores)


def test_render_is_numpys_expression(be):
    rng = np.random.default_rng(3)
    scene = rng.random((37, 53, 4)).astype(np.float32)
    band = scene[:, :, 2]
    got = dm.render_u8(be, dm._Band(be, band, 3, "image")).cpu().numpy().reshape(111, 159)
    big = M.replicate(band, 3)
    assert np.array_equal(got, (big / np.max(big) * 255).astype("uint8")) and got.max() == 255


def test_lidar_matcher_on_the_device_agrees_with_the_emulation(be, tmp_path, capsys):
    from hypelcnn_amd.utilities import lidar_matcher
    from tests.emu_backend import EmuBackend
    results = {}
    for name, backend in (("device", be), ("emulation", EmuBackend())):
        out_dir = tmp_path / name
        results[name] = lidar_matcher.main(CLI + ["--output_path", str(out_dir)], backend=backend)
        check_cli_outputs(results[name], out_dir, capsys.readouterr().out.splitlines())
    device, emulation = results["device"], results["emulation"]
    assert device["top_left"] == emulation["top_left"] and device["bottom_right"] == emulation["bottom_right"]
    assert abs(device["score"] - emulation["score"]) <= (22 * 36 + 16) * M.U24
    assert open(str(tmp_path / "device" / "lidar_match.tif"), "rb").read() == \
        open(str(tmp_path / "emulation" / "lidar_match.tif"), "rb").read()
