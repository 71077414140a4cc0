"""GPU: the grey-scale morphology launches of csrc/morph.hip, MorphologicalProfile and classic_ml_trainer --emp_radii on
the device against the brute-force reference of tests/morph_cases.py -- the cases and checks of tests/test_morph_emu.py,
bit for bit (numpy.array_equal, no tolerance): every input dense and as the interior of a padded, NaN-filled scene whose
origin is 4-byte aligned only, every output between sentinel bytes, every launch twice with equal bits; one tile past a
grid pass; the trainer on the device against the same run on the NumPy twin."""
import numpy as np
import pytest

from hypelcnn_amd.backend import MORPH_DILATE, MORPH_MAX_BLOCKS, MORPH_TILE_H, MORPH_TILE_W
from hypelcnn_amd.classic.morphology import MorphologicalProfile
from hypelcnn_amd.classify import classic_ml_trainer as T
from tests import morph_cases as MC
from tests import test_morph_emu as E
from tests.emu_backend import EmuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.mark.parametrize("h,w,c", MC.SIZES)
def test_erode_dilate(be, h, w, c):
    E.check_erode_dilate(be, h, w, c)


@pytest.mark.parametrize("method", ["dilation", "erosion"])
@pytest.mark.parametrize("case", E.SWEEP_CASES)
def test_sweeps(be, case, method):
    E.check_sweeps(be, case, method)


def test_store(be):
    E.check_store(be)


def test_class_level(be):
    E.check_class_level(be)


def test_one_tile_past_a_grid_pass(be):
    """c = 1 and one tile across: HYPEL_MORPH_MAX_BLOCKS + 1 tiles, so block 0 of both raster kernels takes a second tile,
    the last one, which is two rows short of a whole tile."""
    h, w = MORPH_TILE_H * (MORPH_MAX_BLOCKS + 1) - 2, MORPH_TILE_W
    x = MC.image("normal", h, w, 1, seed=3)
    k = MC.keys_of(x)
    keys, keys_d = MC.run_keys(be, x.reshape(-1), 0, h, w, 1, w, 1)
    assert np.array_equal(keys, k)
    for op in MC.OPS:
        got = MC.run_erode_dilate(be, keys_d, h, w, 1, 2, "disk", op)
        assert np.array_equal(got, MC.ref_erode_dilate(k, 2, "disk", op)), op
    # half of the pixels at their mask already: the limit is a few one-pixel steps away and the reference stays quick
    marker = np.where(np.random.default_rng(4).random(k.shape) < 0.5, k, MC.ref_erode_dilate(k, 1, "square", "erode"))
    limit, steps = MC.ref_reconstruct(marker, k, "dilation")
    out, word = MC.run_sweep(be, marker, k, "dilation")
    MC.check_sweep_contract(marker, k, "dilation", out, word, limit)
    assert not np.array_equal(out[-MORPH_TILE_H:], marker[-MORPH_TILE_H:])  # the last tile was swept
    result, sweeps = MorphologicalProfile((1,), backend=be)._reconstruct(MC.upload_keys(be, marker), keys_d, h, w, 1, MORPH_DILATE,
                                                                            "tail")
    assert np.array_equal(MC.host_keys(result).reshape(h, w, 1), limit)
    print(f"{h} x {w}: {steps} one-pixel steps, {sweeps} sweeps")


@pytest.mark.parametrize("path", [E.SMALL, E.SMALL + ":lidar=0", E.SMALL + ":device=1"])
def test_rows_cut_from_the_profiled_scene(be, path):
    E.check_rows_cut_from_the_profiled_scene(be, path)


def test_the_two_resolution_scene_is_refused_by_name(be):
    with pytest.raises(NotImplementedError, match="two-resolution.*GRSS2018"):
        MorphologicalProfile((1, 2), backend=be).transform_scene(E.data_set("grss2018hr:bands=8:classes=4:h=20:w=24"))


def test_trainer_on_the_device_equals_the_emulation(be, tmp_path):
    """The twins are bit-exact, so the profiled scene and the gathered rows of the two runs are the same bytes; the
    forest grown on the same bytes and its serving are bit-identical between device and emulation
    (tests/test_gpu_forest.py), so the validation labels and the scene raster are held to equality as well."""
    runs = {}
    for name, backend in (("device", be), ("emulation", EmuBackend())):
        log = tmp_path / name
        flags, _ = T.build_parser().parse_known_args(["--emp_radii", "1,2", "--base_log_path", str(log / "direct")] + E.COMMON)
        _, scene, loader = T.compute_profile(flags, backend)
        samples = loader.load_samples(0.1, 0)
        training = T.cut_profiled_patches(scene, samples.training_targets, backend)
        validation = T.cut_profiled_patches(scene, samples.validation_targets, backend)
        est, predicted, _, _, raster = E.run_trainer(backend, log, [])[0]
        report = E.check_report(log, 9)
        assert est.n_features_in_ == 25 * 9 * 5 and raster.shape == (20, 24)
        runs[name] = (scene.casi_dev.cpu().numpy(), training.data, validation.data, np.asarray(predicted), raster)
        print(name, "sweeps per level", report["sweeps"], "seconds", round(report["seconds"], 4))
    for what, a, b in zip(("scene", "training rows", "validation rows", "labels", "raster"), runs["device"], runs["emulation"]):
        assert E.same(a, b), what
    assert len(np.unique(runs["device"][4])) > 1
    est = E.run_trainer(be, tmp_path / "pca", ["--pca_components", "4"])[0][0]
    assert est.n_features_in_ == 25 * (4 + 1) * 5
    E.check_report(tmp_path / "pca", 5)
