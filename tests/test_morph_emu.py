"""CPU: the NumPy twins of the hypel_morph_* entry points (tests/emu_morph.py), hypelcnn_amd.classic.morphology.
MorphologicalProfile and the --emp_* flags of classify/classic_ml_trainer.py against the brute-force reference of
tests/morph_cases.py, bit for bit; scipy.ndimage's grey erosion / dilation where scipy is installed.  The check_*
functions take a backend: tests/test_gpu_morph.py asks the same of the device."""
import json
import os

import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import MORPH_MAX_RADIUS, Ref
from hypelcnn_amd.classic.decomposition import BandPCA, ProjectedScene
from hypelcnn_amd.classic.morphology import MorphologicalProfile
from hypelcnn_amd.classify import classic_ml_trainer as T
from hypelcnn_amd.common.common_nn_ops import SceneArrays, get_loader_from_name
from tests import emu_forest, emu_morph, emu_pca, emu_scene, emu_svm  # noqa: F401 -- attach the emulations to EmuBackend
from tests import morph_cases as MC
from tests.emu_backend import EmuBackend

SMALL = "grss2013:bands=8:classes=4:h=20:w=24"
COMMON = ["--loader_name", "SyntheticDataLoader", "--path", SMALL, "--neighborhood", "2"]
SWEEP_CASES = ("random", "above", "limit", "constant", "serpentine")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(MC.bits(a), MC.bits(b))


# ------------------------------------------------------------------------------------------------------- launches
def check_erode_dilate(be, h, w, c):
    for kind in MC.VALUES:
        x = MC.image(kind, h, w, c)
        for name, buf, origin, stride_y, stride_x in MC.layouts(x):
            keys, keys_d = MC.run_keys(be, buf, origin, h, w, c, stride_y, stride_x)
            assert np.array_equal(keys, MC.keys_of(x)), (kind, name)
            assert same(MC.floats_of(keys), x)  # the inverse mapping is exact, NaN payloads included
            for radius in MC.RADII:
                for shape in MC.SHAPES:
                    for op in MC.OPS:
                        _, want = MC.erode_dilate_case(kind, h, w, c, radius, shape, op)
                        got = MC.run_erode_dilate(be, keys_d, h, w, c, radius, shape, op)
                        assert np.array_equal(got, want), (kind, name, radius, shape, op)
                        again = MC.run_erode_dilate(be, keys_d, h, w, c, radius, shape, op)
                        assert np.array_equal(again, got), (kind, name, radius, shape, op)


@pytest.mark.parametrize("h,w,c", MC.SIZES)
def test_erode_dilate(h, w, c):
    check_erode_dilate(EmuBackend(), h, w, c)


def test_the_reference_is_scipys_grey_erosion_and_dilation():
    """on inputs without signed zeros or NaN (+-inf present): the definition the reference and the twin share is sound"""
    ndimage = pytest.importorskip("scipy.ndimage")
    be = EmuBackend()
    x = MC.image("normal", 37, 45, 1)
    x[3, 4], x[20, 30], x[36, 44] = np.inf, -np.inf, np.inf
    keys_d = MC.upload_keys(be, MC.keys_of(x))
    for radius in (1, 2, 7):
        for shape in MC.SHAPES:
            footprint = np.zeros((2 * radius + 1, 2 * radius + 1), bool)
            for dy, dx in MC.offsets(radius, shape):
                footprint[dy + radius, dx + radius] = True
            for op, fn, cval in (("erode", ndimage.grey_erosion, np.inf), ("dilate", ndimage.grey_dilation, -np.inf)):
                theirs = fn(x[:, :, 0], footprint=footprint, mode="constant", cval=cval)
                assert same(MC.floats_of(MC.ref_erode_dilate(MC.keys_of(x), radius, shape, op))[:, :, 0], theirs)
                assert same(MC.floats_of(MC.run_erode_dilate(be, keys_d, 37, 45, 1, radius, shape, op))[:, :, 0], theirs)


def test_the_serpentine_of_the_reference_fills():
    marker, mask = MC.serpentine(41, 41)
    limit, steps = MC.ref_reconstruct(MC.keys_of(marker), MC.keys_of(mask), "dilation")
    assert same(MC.floats_of(limit), mask) and steps == 840


def sweep_case(case, method):
    """(marker keys, mask keys) of a case; the erosion cases are the dilation cases under k -> ~k, which reverses the order"""
    rng = np.random.default_rng(SWEEP_CASES.index(case))
    if case == "serpentine":
        marker, mask = MC.serpentine(130, 70)  # 64 x 16 tiles: the corridor crosses tile borders in both directions
    else:
        mask = rng.standard_normal((40, 70, 3)).astype(np.float32)
        if case == "constant":
            mask[...] = 0.25
        marker = mask - np.abs(rng.standard_normal(mask.shape)).astype(np.float32) * (rng.random(mask.shape) < 0.9)
        if case == "above":
            marker = mask + rng.standard_normal(mask.shape).astype(np.float32)  # about half of it lies above its mask
    marker, mask = MC.keys_of(marker), MC.keys_of(mask)
    if case == "limit":
        marker = MC.ref_reconstruct(marker, mask, "dilation")[0]
    return (marker, mask) if method == "dilation" else (~marker, ~mask)


def check_sweeps(be, case, method):
    marker, mask = sweep_case(case, method)
    h, w, c = marker.shape
    limit, steps = MC.ref_reconstruct(marker, mask, method)
    if case == "above":
        assert (marker > mask).any() and (marker < mask).any()
    if case == "limit":
        assert np.array_equal(marker, limit) and steps == 0
    state = marker
    for _ in range(3):  # the first launches, each held to the four clauses on its own
        out, word = MC.run_sweep(be, state, mask, method)
        MC.check_sweep_contract(state, mask, method, out, word, limit)
        again, _ = MC.run_sweep(be, state, mask, method)
        assert np.array_equal(again, out)
        if case == "limit":
            assert word == 0 and np.array_equal(out, marker)
        state = out
    _, word = MC.run_sweep(be, limit, mask, method, flag=1)  # the word is never cleared
    assert word == 1
    profile = MorphologicalProfile((1,), backend=be)
    op = emu_morph.MORPH_DILATE if method == "dilation" else emu_morph.MORPH_ERODE
    result, sweeps = profile._reconstruct(MC.upload_keys(be, marker), MC.upload_keys(be, mask), h, w, c, op, case)
    assert np.array_equal(MC.host_keys(result).reshape(h, w, c), limit)
    print(f"reconstruction by {method}, {case} {h} x {w} x {c}: {steps} one-pixel steps, the driver launched {sweeps} sweeps")


@pytest.mark.parametrize("method", ["dilation", "erosion"])
@pytest.mark.parametrize("case", SWEEP_CASES)
def test_sweeps(case, method):
    check_sweeps(EmuBackend(), case, method)


def check_store(be):
    x = MC.image("special", 7, 9, 3)
    k = MC.keys_of(x)
    for pad in (0, 1, 2, 5):
        got = MC.run_store(be, k, pad, 8, 1, 2)  # bases to channels 1, 3, 5 of 8
        want = np.full((7 + 2 * pad, 9 + 2 * pad, 8), MC.SENTINEL * 0x01010101, np.uint32)
        want[:, :, 1:6:2] = np.pad(x.view(np.uint32), ((pad, pad), (pad, pad), (0, 0)), mode="symmetric")
        assert np.array_equal(got, want), pad
    small = MC.keys_of(MC.image("special", 2, 3, 1))  # pad == min(h, w): the whole image reflected once
    assert np.array_equal(MC.run_store(be, small, 2, 1, 0, 1), np.pad(MC.floats_of(small).view(np.uint32),
                                                                     ((2, 2), (2, 2), (0, 0)), mode="symmetric"))
    dense = MC.run_store(be, k, 0, 3, 0, 1)
    assert same(dense.view(np.float32), x)  # the key round trip gives back the input's bits


def test_store():
    check_store(EmuBackend())


def test_the_twins_refuse_what_the_library_refuses():
    be = EmuBackend()
    k = MC.upload_keys(be, MC.keys_of(MC.image("normal", 4, 5, 2)))
    out, flag = be.empty(4000, torch.int32), be.zeros(1, torch.int32)
    floats = be.empty(4000)
    bad = [("morph_erode_dilate_u32", (Ref(k), 4, 5, 2, MORPH_MAX_RADIUS + 1, 0, 0, Ref(out))),
           ("morph_erode_dilate_u32", (Ref(k), 4, 5, 2, -1, 0, 0, Ref(out))),
           ("morph_erode_dilate_u32", (Ref(k), 4, 5, 2, 1, 2, 0, Ref(out))),
           ("morph_erode_dilate_u32", (Ref(k), 4, 5, 2, 1, 0, 2, Ref(out))),
           ("morph_erode_dilate_u32", (Ref(k), 0, 5, 2, 1, 0, 0, Ref(out))),
           ("morph_erode_dilate_u32", (Ref(k), 4, 5, 0, 1, 0, 0, Ref(out))),
           ("morph_erode_dilate_u32", (Ref(k), 4, 5, 2, 1, 0, 0, Ref(k))),
           ("morph_erode_dilate_u32", (None, 4, 5, 2, 1, 0, 0, Ref(out))),
           ("morph_reconstruct_sweep_u32", (Ref(k), Ref(k), 4, 5, 2, 2, Ref(out), Ref(flag))),
           ("morph_reconstruct_sweep_u32", (Ref(k), Ref(k), 4, 5, 2, 1, Ref(k), Ref(flag))),
           ("morph_reconstruct_sweep_u32", (Ref(k), Ref(k), 4, 5, 2, 1, Ref(out), None)),
           ("morph_profile_store_f32", (Ref(k), 4, 5, 2, 5, Ref(floats), 2, 0, 1)),   # a pad larger than h
           ("morph_profile_store_f32", (Ref(k), 4, 5, 2, -1, Ref(floats), 2, 0, 1)),
           ("morph_profile_store_f32", (Ref(k), 4, 5, 2, 1, Ref(floats), 2, 1, 1)),   # the last base leaves out_c
           ("morph_profile_store_f32", (Ref(k), 4, 5, 2, 1, Ref(floats), 4, 0, 0)),
           ("morph_keys_u32", (Ref(floats), 4, 5, 2, 10, 1, Ref(out))),               # stride_x below c
           ("morph_keys_u32", (Ref(floats), 4, 5000, 2, 10000, 2, Ref(out)))]         # the view leaves its buffer
    for name, args in bad:
        with pytest.raises(AssertionError):
            be.call(name, *args)


# ------------------------------------------------------------------------------------------------------- the class
def check_class_level(be):
    x = MC.image("normal", 40, 50, 3, seed=5)
    k = MC.keys_of(x)
    for by_reconstruction in (True, False):
        profile = MorphologicalProfile((1, 3), by_reconstruction=by_reconstruction, backend=be)
        got = profile.transform(x)
        want = MC.ref_profile(x, (1, 3), "disk", by_reconstruction)
        assert isinstance(got, np.ndarray) and got.shape == (40, 50, 15) and got.dtype == np.float32
        for channel in range(15):
            assert same(got[:, :, channel], want[:, :, channel]), (by_reconstruction, channel)
        assert same(got[:, :, 2::5], x)  # the base itself sits in the middle of its five channels
        assert set(profile.sweeps_) == ({f"image/{kind}/{r}" for kind in ("opening", "closing") for r in (1, 3)}
                                        if by_reconstruction else set())
        for r in (1, 3):
            assert same(profile.opening(x, r), MC.floats_of(MC.ref_opening(k, r, "disk", by_reconstruction)))
            assert same(profile.closing(x, r), MC.floats_of(MC.ref_closing(k, r, "disk", by_reconstruction)))
    profile = MorphologicalProfile((2,), shape="square", backend=be)
    assert profile.get_params() == {"radii": [2], "shape": "square", "by_reconstruction": True, "include_lidar": True}
    for r in (0, 2, 3):
        assert same(profile.erode(x, r), MC.floats_of(MC.ref_erode_dilate(k, r, "square", "erode")))
        assert same(profile.dilate(x[:, :, 0], r), MC.floats_of(MC.ref_erode_dilate(k[:, :, :1], r, "square", "dilate"))[:, :, 0])
        # duality phi_r(f) = -gamma_r(-f): negation reverses the order exactly (a NaN-free input)
        assert same(profile.closing(x, r), -profile.opening(-x, r))
        # gamma_r^rec(f) <= f, and it restores at least what the plain opening does
        opened = MC.keys_of(profile.opening(x, r))
        plain = MC.ref_erode_dilate(MC.ref_erode_dilate(k, r, "square", "erode"), r, "square", "dilate")
        assert (opened <= k).all() and (opened >= plain).all()
    marker = (x - 1.0).astype(np.float32)
    for method in ("dilation", "erosion"):
        sign = 1.0 if method == "dilation" else -1.0
        want = MC.floats_of(MC.ref_reconstruct(MC.keys_of(sign * marker), MC.keys_of(sign * x), method)[0])
        assert same(profile.reconstruct(sign * marker, sign * x, method), want)
    # a device tensor in gives a device tensor out; a strided view -- the interior of a padded scene with a trailing
    # channel, NaN around it -- is read in place
    scene = torch.full((44, 54, 4), float("nan"), device=be.device)
    scene[2:42, 2:52, :3] = torch.from_numpy(x).to(be.device)
    view = scene[2:42, 2:52, :3]
    assert not view.is_contiguous()
    for got, want in ((profile.erode(view, 2), profile.erode(x, 2)), (profile.transform(view), profile.transform(x)),
                      (profile.opening(view, 3), profile.opening(x, 3))):
        assert isinstance(got, torch.Tensor) and got.device.type == be.device.type and same(got.cpu().numpy(), want)


def test_class_level():
    check_class_level(EmuBackend())


def test_every_refusal_by_name():
    be = EmuBackend()
    for bad in ((), (0,), (MORPH_MAX_RADIUS + 1,), (2, 2), (3, 2), (1.5,), (True,), ("2",), (-1, 2)):
        with pytest.raises(ValueError, match="radii"):
            MorphologicalProfile(bad, backend=be)
    assert MorphologicalProfile(3, backend=be).radii == (3,)
    assert MorphologicalProfile([1, MORPH_MAX_RADIUS], backend=be).radii == (1, MORPH_MAX_RADIUS)
    with pytest.raises(ValueError, match="shape='hexagon'"):
        MorphologicalProfile((1,), shape="hexagon", backend=be)
    profile = MorphologicalProfile((1,), backend=be)
    x = MC.image("normal", 6, 7, 2)
    for bad in (-1, MORPH_MAX_RADIUS + 1, 1.0, True):
        with pytest.raises(ValueError, match="HYPEL_MORPH_MAX_RADIUS"):
            profile.erode(x, bad)
    with pytest.raises(ValueError, match="method='opening'"):
        profile.reconstruct(x, x, "opening")
    with pytest.raises(ValueError, match="a marker of shape"):
        profile.reconstruct(x[:, :, :1], x)
    with pytest.raises(ValueError, match=r"\[h, w\] or \[h, w, channels\]"):
        profile.erode(np.zeros((2, 2, 2, 2), np.float32), 1)
    with pytest.raises(ValueError, match="NumPy array or a device tensor"):
        profile.erode([[1.0]], 1)
    from hypelcnn_amd.loader.GULFPORTALTDataLoader import MultiDataSet
    with pytest.raises(NotImplementedError, match="MultiDataSet.*GULFPORTALT"):
        profile.transform_scene(MultiDataSet(data_set(SMALL), data_set(SMALL)))
    with pytest.raises(NotImplementedError, match="two-resolution.*GRSS2018"):
        profile.transform_scene(data_set("grss2018hr:bands=8:classes=4:h=20:w=24"))


def test_the_driver_names_the_level_that_does_not_settle(monkeypatch):
    """a sweep that always reports a change: the driver gives up after h * w sweeps (and the two groups on top)"""
    be = EmuBackend()

    def restless(self, marker_in, mask, h, w, c, op, marker_out, changed):
        self.launch_log.append("morph_reconstruct_sweep_u32")
        emu_morph._arr(changed, np.int32)[0] = 1
    monkeypatch.setattr(EmuBackend, "k_morph_reconstruct_sweep_u32", restless)
    with pytest.raises(RuntimeError, match=r"level image/opening/1.*3 x 4 raster did not settle in 20 sweeps"):
        MorphologicalProfile((1,), backend=be).transform(MC.image("normal", 3, 4, 1))


# ------------------------------------------------------------------------------------------------------- scenes
def data_set(path, neighborhood=2, be=None):
    loader = get_loader_from_name("SyntheticDataLoader", path)
    loader.backend = be
    return loader.load_data(neighborhood, False)


def check_rows_cut_from_the_profiled_scene(be, path):
    """rows gathered from the profiled scene == windows of the brute-force profile of the interior, re-padded"""
    ds = data_set(path, be=be)
    casi, lidar = (None if t is None else t.cpu().numpy() for t in SceneArrays._resident(ds, be.device))
    h, w = ds.get_scene_shape()
    assert casi.shape[:2] == (h + 4, w + 4)
    points = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + [(int(x), int(y)) for x, y in
                                                                 np.random.default_rng(1).integers(0, (w, h), (12, 2))]
    targets = np.array([(x, y, 0) for x, y in points])
    index = torch.arange(len(targets), device=be.device)
    for include_lidar in (True, False):
        profile = MorphologicalProfile((1, 2), include_lidar=include_lidar, backend=be)
        scene = profile.transform_scene(ds)
        bases = [casi[2:-2, 2:-2, :]] + ([lidar[2:-2, 2:-2, :]] if include_lidar and lidar is not None else [])
        want = np.pad(MC.ref_profile(np.concatenate(bases, axis=2), (1, 2)), ((2, 2), (2, 2), (0, 0)), mode="symmetric")
        assert isinstance(scene, ProjectedScene) and same(scene.casi_dev.cpu().numpy(), want)
        if include_lidar or lidar is None:
            assert scene.lidar_dev is None
        else:
            assert same(scene.lidar_dev.cpu().numpy(), lidar)
            want = np.concatenate([want, lidar], axis=2)
        assert scene.get_data_shape() == [5, 5, want.shape[2]] and scene.get_scene_shape() == [h, w]
        assert scene.get_casi_band_count() == 5 * sum(b.shape[2] for b in bases) and scene.neighborhood == 2
        arrays = SceneArrays()
        arrays.feed(scene, targets, be)
        cut, _ = arrays.gather(index)
        for (x, y), patch in zip(points, cut.cpu().numpy()):
            assert same(patch, want[y:y + 5, x:x + 5, :]), (include_lidar, x, y)
    # behind a band PCA: the ProjectedScene it returns is read like any other scene
    pca = BandPCA(3, backend=be).fit_scene(ds)
    projected = pca.transform_scene(ds)
    scene = MorphologicalProfile((2,), backend=be).transform_scene(projected)
    bases = [projected.casi_dev.cpu().numpy()[2:-2, 2:-2, :]] + ([] if lidar is None else [lidar[2:-2, 2:-2, :]])
    want = np.pad(MC.ref_profile(np.concatenate(bases, axis=2), (2,)), ((2, 2), (2, 2), (0, 0)), mode="symmetric")
    assert same(scene.casi_dev.cpu().numpy(), want)


@pytest.mark.parametrize("path", [SMALL, SMALL + ":lidar=0", SMALL + ":device=1"])
def test_rows_cut_from_the_profiled_scene(path):
    check_rows_cut_from_the_profiled_scene(EmuBackend(), path)


# ------------------------------------------------------------------------------------------------------- the trainer
def outputs(directory):
    return {name: open(os.path.join(directory, name), "rb").read() for name in sorted(os.listdir(directory))}


def run_trainer(backend, log, extra):
    return T.main(["--estimator", "forest", "--forest_trees", "8", "--emp_radii", "1,2", "--fullscene", "--base_log_path",
                   str(log), "--output_path", str(log)] + extra + COMMON, backend=backend)


def check_report(log, bases, by_reconstruction=True):
    report = json.load(open(os.path.join(log, "emp_SyntheticDataLoader.json")))
    assert set(report) == {"radii", "shape", "by_reconstruction", "include_lidar", "bases", "channels", "sweeps", "seconds"}
    assert (report["radii"], report["shape"], report["by_reconstruction"], report["include_lidar"]) == \
        ([1, 2], "disk", by_reconstruction, True)
    assert report["bases"] == bases and report["channels"] == 5 * bases and report["seconds"] >= 0
    names = {f"{raster}/{kind}/{r}" for raster in ("hsi", "lidar") for kind in ("opening", "closing") for r in (1, 2)}
    assert set(report["sweeps"]) == (names if by_reconstruction else set())
    assert all(isinstance(v, int) and v >= 4 and v % 4 == 0 for v in report["sweeps"].values())
    return report


@pytest.mark.parametrize("estimator", T.ESTIMATORS)
def test_trainer_with_each_estimator(estimator, tmp_path):
    be = EmuBackend()
    log, out = tmp_path / "log", tmp_path / "out"
    result = T.main(["--estimator", estimator, "--forest_trees", "4", "--emp_radii", "1,2", "--fullscene", "--split_count", "2",
                     "--base_log_path", str(log), "--output_path", str(out)] + COMMON, backend=be)
    est, predicted, cm, _, scene = result[1]
    features = est.n_features_in_ if hasattr(est, "n_features_in_") else est._f
    assert features == 25 * (8 + 1) * 5 and scene.shape == (20, 24) and cm.sum() == len(predicted)
    # once per process: one keys launch per raster, whatever the episodes and --fullscene ask
    assert be.launch_log.count("morph_keys_u32") == 2 and be.launch_log.count("morph_erode_dilate_u32") == 2 * 4
    assert be.launch_log.count("morph_profile_store_f32") == 2 * 5
    check_report(log, 9)
    assert os.path.exists(out / "result_raw.tif") and os.path.exists(log / "metrics_SyntheticDataLoader_run1.txt")


def test_trainer_behind_the_pca_plain_square_without_lidar_and_diagnostics(tmp_path):
    be = EmuBackend()
    result = run_trainer(be, tmp_path / "a", ["--pca_components", "4"])
    assert result[0][0].n_features_in_ == 25 * (4 + 1) * 5
    check_report(tmp_path / "a", 5)
    assert be.launch_log.index("pca_project_f32") < be.launch_log.index("morph_keys_u32")
    assert be.launch_log.count("pca_project_f32") == 1  # the scene once; no patch is projected on the host side
    result = run_trainer(be, tmp_path / "b", ["--emp_plain", "--emp_shape", "square", "--emp_lidar", "false",
                                              "--forest_importances"])
    assert result[0][0].n_features_in_ == 25 * (8 * 5 + 1)
    report = json.load(open(tmp_path / "b" / "emp_SyntheticDataLoader.json"))
    assert (report["shape"], report["by_reconstruction"], report["include_lidar"], report["bases"], report["sweeps"]) == \
        ("square", False, False, 8, {})
    # the band axis of the diagnostics means profile channels (+ the LiDAR channel that passed through)
    assert np.load(tmp_path / "b" / "feature_importance_SyntheticDataLoader_run0.npy").shape == (5, 5, 41)
    for bad in ("x", "1,,x", "2;4"):
        with pytest.raises(SystemExit):
            T.main(["--emp_radii", bad] + COMMON, backend=EmuBackend())
    with pytest.raises(ValueError, match="radii"):
        T.main(["--emp_radii", "4,2"] + COMMON, backend=EmuBackend())
    with pytest.raises(NotImplementedError, match="two-resolution"):
        T.main(["--emp_radii", "2", "--loader_name", "SyntheticDataLoader", "--path", "grss2018hr:bands=8:classes=4:h=20:w=24",
                "--neighborhood", "2", "--base_log_path", str(tmp_path / "c")], backend=EmuBackend())


def test_the_training_rows_are_cut_from_the_profiled_scene(tmp_path):
    be = EmuBackend()
    flags, _ = T.build_parser().parse_known_args(["--emp_radii", "1,2", "--base_log_path", str(tmp_path)] + COMMON)
    profile, scene, loader = T.compute_profile(flags, be)
    ds = data_set(SMALL)
    want = np.pad(MC.ref_profile(np.concatenate([ds.casi[2:-2, 2:-2], ds.lidar[2:-2, 2:-2]], axis=2), (1, 2)),
                  ((2, 2), (2, 2), (0, 0)), mode="symmetric")
    sample_set = loader.load_samples(0.1, 0)
    rows = T.cut_profiled_patches(scene, sample_set.training_targets, be)
    assert rows.data.shape == (len(sample_set.training_targets), 5, 5, 45) and rows.labels.dtype == np.uint8
    assert np.array_equal(rows.labels, sample_set.training_targets[:, 2])
    for (x, y, _), patch in zip(sample_set.training_targets, rows.data):
        assert same(patch, want[y:y + 5, x:x + 5])


def test_trainer_without_the_flag_runs_what_it_ran_before(tmp_path, capsys):
    """the flag parsed but empty against the flag absent: the same launches, files and printed lines"""
    runs = {}
    for name, extra in (("without", []), ("empty", ["--emp_radii", ""]), ("bare", ["--emp_radii"])):
        be = EmuBackend()
        capsys.readouterr()
        T.main(["--estimator", "forest", "--forest_trees", "4", "--fullscene", "--base_log_path", str(tmp_path / name / "log"),
                "--output_path", str(tmp_path / name / "out")] + extra + COMMON, backend=be)
        printed = [line for line in capsys.readouterr().out.splitlines() if "sec)" not in line]  # (wall-clock lines)
        runs[name] = (be.launch_log, outputs(tmp_path / name / "log"), outputs(tmp_path / name / "out"), printed)
    assert runs["empty"] == runs["without"] and runs["bare"] == runs["without"]
    assert not any(entry.startswith("morph_") for entry in runs["without"][0])
    assert not any(name.startswith("emp_") for name in runs["without"][1])
