"""CPU: hypelcnn_amd.classic.decomposition.BandPCA and the --pca_components flags of classify/classic_ml_trainer.py on
the NumPy twins of the hypel_pca_* entry points (tests/emu_pca.py): against numpy.linalg.eigh of the float64 covariance
within the derived bounds of tests/pca_cases.py, scikit-learn's rule for a fractional n_components, the sign convention,
the padding a scene fit must not count, the bits a pixel projects to wherever it lies, every refusal by name,
scikit-learn's PCA where it is installed, and the trainer end to end with each estimator."""
import json
import os

import numpy as np
import pytest
import torch

from hypelcnn_amd.classic.decomposition import BandPCA, ProjectedScene
from hypelcnn_amd.classify import classic_ml_trainer as T
from hypelcnn_amd.common.common_nn_ops import SceneArrays, get_loader_from_name
from tests import emu_forest, emu_pca, emu_scene, emu_svm  # noqa: F401 -- attach the emulations to EmuBackend
from tests import pca_cases as PC
from tests.emu_backend import EmuBackend

SMALL = "grss2013:bands=8:classes=4:h=20:w=24"
COMMON = ["--loader_name", "SyntheticDataLoader", "--path", SMALL, "--neighborhood", "2"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_against_eigh_of_the_float64_covariance():
    x = PC.spectrum_pixels(3000, 12)
    pca = BandPCA(6, backend=EmuBackend()).fit(x)
    assert pca.components_.shape == (6, 12) and pca.mean_.shape == (12,) and pca.explained_variance_.shape == (6,)
    assert (pca.n_components_, pca.n_samples_, pca.n_features_in_) == (6, 3000, 12)
    assert pca.get_params() == {"n_components": 6, "whiten": False}
    PC.check_against_eigh(pca, x)
    assert (np.diff(pca.explained_variance_) < 0).all()
    # a three-dimensional view gives what its rows give
    again = BandPCA(6, backend=EmuBackend()).fit(x.reshape(50, 60, 12))
    assert np.array_equal(bits(again.components_), bits(pca.components_))


def test_hard_data_and_the_float32_mean_correction():
    """Means of 10^4 over standard deviations down to 0.007: without the n / (n - 1) d d^T term the small bands' variances
    are off by what the float32 rounding of the mean adds."""
    x = PC.hard_pixels(4000, 9, seed=5)
    pca = BandPCA(9, backend=EmuBackend()).fit(x)
    x64 = x.astype(np.float64)
    values = np.linalg.eigvalsh(np.cov(x64.T))[::-1]
    d_c = PC.covariance_bound(x, pca.mean_, values[0])
    assert (np.abs(pca.explained_variance_ - np.clip(values, 0, None)) <= d_c).all()
    # the constant band: zero up to eigh's own rounding, and never below (clipped)
    assert 0.0 <= pca.explained_variance_[-1] <= 9 * 2.0 ** -52 * values[0]


def test_fraction_rule_is_scikit_learns():
    x = PC.spectrum_pixels(3000, 12)
    ratio = BandPCA(12, backend=EmuBackend()).fit(x).explained_variance_ratio_
    for share in (0.5, 0.9, 0.95, 0.999, float(np.cumsum(ratio)[2])):
        pca = BandPCA(share, backend=EmuBackend()).fit(x)
        want = int(np.searchsorted(np.cumsum(ratio), share, side="right")) + 1
        assert pca.n_components_ == want and pca.components_.shape == (want, 12)
        assert np.cumsum(ratio)[want - 1] > share and (want == 1 or np.cumsum(ratio)[want - 2] <= share)
    assert BandPCA(0.9, backend=EmuBackend()).fit(x).n_components_ == 2  # 0.75, 0.9375: the spectrum has ratio 4


def test_sign_convention():
    x = PC.spectrum_pixels(2000, 7, seed=3)
    pca = BandPCA(7, backend=EmuBackend()).fit(x)
    lead = np.argmax(np.abs(pca.components_), axis=1)
    assert (pca.components_[np.arange(7), lead] > 0).all()
    # mirrored data: every component changes sign with it, and the convention turns it back
    mirrored = BandPCA(7, backend=EmuBackend()).fit((20000.0 - x).astype(np.float32))
    assert np.abs(mirrored.components_ - pca.components_).max() < 1e-3


def data_set(path, neighborhood=2):
    return get_loader_from_name("SyntheticDataLoader", path).load_data(neighborhood, False)


def test_fit_scene_ignores_the_padding():
    ds = data_set(SMALL)
    on_scene = BandPCA(3, backend=EmuBackend()).fit_scene(ds)
    interior = np.ascontiguousarray(ds.casi[2:-2, 2:-2, :])
    on_interior = BandPCA(3, backend=EmuBackend()).fit(interior)
    assert on_scene.n_samples_ == 20 * 24
    for name in ("mean_", "components_", "explained_variance_", "explained_variance_ratio_"):
        assert np.array_equal(bits(getattr(on_scene, name)), bits(getattr(on_interior, name))), name
    padded = BandPCA(3, backend=EmuBackend()).fit(ds.casi)  # counting the reflections gives another answer
    assert not np.array_equal(padded.mean_, on_scene.mean_)


@pytest.mark.parametrize("path", ["grss2013:bands=8:classes=4:h=20:w=24", "grss2013:bands=8:classes=4:h=20:w=24:lidar=0",
                                  "grss2018hr:bands=8:classes=4:h=20:w=24"])
def test_rows_cut_from_the_projected_scene_are_the_projected_rows(path):
    check_rows_cut_from_the_projected_scene(EmuBackend(), path)


def check_rows_cut_from_the_projected_scene(be, path):
    """(also what tests/test_gpu_pca.py asks of the device)"""
    ds = data_set(path)
    pca = BandPCA(3, backend=be).fit_scene(ds)
    scene = pca.transform_scene(ds)
    lidar = 0 if ds.lidar is None else 1
    assert isinstance(scene, ProjectedScene) and tuple(scene.casi_dev.shape) == ds.casi.shape[:2] + (3,)
    assert scene.get_data_shape() == [5, 5, 3 + lidar] and scene.get_scene_shape() == ds.get_scene_shape()
    assert scene.neighborhood == 2 and scene.casi_scale == getattr(ds, "casi_scale", 1)
    assert (scene.lidar_dev is None) == (ds.lidar is None)
    if lidar:
        assert np.array_equal(scene.lidar_dev.cpu().numpy(), ds.lidar.astype(np.float32))
    h, w = ds.get_scene_shape()
    rng = np.random.default_rng(1)
    points = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + [(int(rng.integers(w)), int(rng.integers(h))) for _ in range(12)]
    targets = np.array([(x, y, 0) for x, y in points])
    index = torch.arange(len(targets), device=be.device)
    raw, projected = SceneArrays(), SceneArrays()
    raw.feed(ds, targets, be)
    projected.feed(scene, targets, be)
    patches, _ = raw.gather(index)          # [b, 5, 5, 8 + lidar]
    cut, _ = projected.gather(index)        # [b, 5, 5, 3 + lidar]
    rows = pca.transform(patches.cpu().numpy().reshape(-1, 8 + lidar), pass_cols=lidar)
    assert rows.shape == (len(targets) * 25, 3 + lidar)
    assert np.array_equal(bits(cut.cpu().numpy().reshape(-1, 3 + lidar)), bits(rows))
    # a device tensor comes back as one, with the same bits
    as_tensor = pca.transform(patches.reshape(-1, 8 + lidar), pass_cols=lidar)
    assert isinstance(as_tensor, torch.Tensor) and np.array_equal(bits(as_tensor.cpu().numpy()), bits(rows))


def test_whitened_components_have_unit_variance():
    x = PC.spectrum_pixels(3000, 12)
    pca = BandPCA(5, whiten=True, backend=EmuBackend()).fit(x)
    out = pca.transform(x).astype(np.float64)
    weights = (pca.components_ / np.sqrt(pca.explained_variance_)[:, None]).T.astype(np.float32)
    mean32 = pca.mean_.astype(np.float32)
    _, bound = PC.projection_bound(x, 12, mean32, weights)
    # the rows are centred on the float32 mean: the column means are what its rounding projects to, + the rounding
    off = np.abs(pca.mean_ - mean32.astype(np.float64)) @ np.abs(weights.astype(np.float64)) + bound.mean(0)
    assert (np.abs(out.mean(0)) <= off + 1e-12).all()
    # variances: the float64 projection has variance v' W^T C W v' = 1 up to the relative error of the eigenvalue and
    # twice the component's turn (tests/pca_cases.py); the rounding adds at most twice its bound over the unit spread
    values = np.linalg.eigvalsh(np.cov(x.astype(np.float64).T))[::-1]
    d_c = PC.covariance_bound(x, pca.mean_, values[0])
    for j in range(5):
        gap = np.abs(np.delete(values, j) - values[j]).min()
        slack = d_c / values[j] + 2 * (2 * d_c / gap) * values[0] / values[j] + 3 * bound[:, j].max()
        assert abs(out[:, j].var(ddof=1) - 1) <= slack, j


def test_every_refusal_by_name():
    be = EmuBackend()
    for bad in (0, -1, 1.0, 1.5, 0.0, "3", True, None):
        with pytest.raises(ValueError, match="n_components"):
            BandPCA(bad, backend=be)
    x = PC.spectrum_pixels(100, 6)
    with pytest.raises(ValueError, match="n_components=7 of 6 bands"):
        BandPCA(7, backend=be).fit(x)
    with pytest.raises(ValueError, match="at least 2"):
        BandPCA(1, backend=be).fit(x[:1])
    with pytest.raises(ValueError, match="HYPEL_PCA_MAX_BANDS"):
        BandPCA(1, backend=be).fit(np.zeros((4, 513), np.float32))
    with pytest.raises(ValueError, match=r"\[rows, bands\] or \[h, w, bands\]"):
        BandPCA(1, backend=be).fit(np.zeros((2, 2, 2, 2), np.float32))
    flat = x.copy()
    flat[:, 1:] = 7.0
    with pytest.raises(ValueError, match=r"whiten=True.*component 1 .*zero variance"):
        BandPCA(2, whiten=True, backend=be).fit(flat)
    assert BandPCA(2, backend=be).fit(flat).explained_variance_[1] == 0.0
    pca = BandPCA(2, backend=be)
    with pytest.raises(ValueError, match="fit first"):
        pca.transform(x)
    with pytest.raises(ValueError, match="fit first"):
        pca.transform_scene(data_set(SMALL))
    pca.fit(x)
    with pytest.raises(ValueError, match="5 bands, the model was fitted on 6"):
        pca.transform(x[:, :5])
    with pytest.raises(ValueError, match="5 bands, the model was fitted on 6"):
        pca.transform(x, pass_cols=1)
    with pytest.raises(ValueError, match="pass_cols"):
        pca.transform(x, pass_cols=-1)
    with pytest.raises(ValueError, match="8 bands, the model was fitted on 6"):
        pca.transform_scene(data_set(SMALL))
    from hypelcnn_amd.loader.GULFPORTALTDataLoader import MultiDataSet
    several = MultiDataSet(data_set(SMALL), data_set(SMALL))
    with pytest.raises(NotImplementedError, match="MultiDataSet.*GULFPORTALT"):
        BandPCA(2, backend=be).fit_scene(several)
    with pytest.raises(NotImplementedError, match="MultiDataSet.*GULFPORTALT"):
        pca.transform_scene(several)
    assert pca.transform(x[:0]).shape == (0, 2)


def test_against_scikit_learn():
    decomposition = pytest.importorskip("sklearn.decomposition")
    x = PC.spectrum_pixels(3000, 12)
    x64 = x.astype(np.float64)
    for whiten in (False, True):
        ours = BandPCA(5, whiten=whiten, backend=EmuBackend()).fit(x)
        theirs = decomposition.PCA(5, whiten=whiten, svd_solver="full").fit(x64)
        d_c = PC.covariance_bound(x, ours.mean_, theirs.explained_variance_[0])
        assert (np.abs(ours.explained_variance_ - theirs.explained_variance_) <= d_c).all()
        assert np.allclose(ours.explained_variance_ratio_, theirs.explained_variance_ratio_, rtol=1e-5)
        values = np.linalg.eigvalsh(np.cov(x64.T))[::-1]
        sign = np.sign(np.sum(ours.components_ * theirs.components_, axis=1))
        got = ours.transform(x).astype(np.float64)
        want = theirs.transform(x64) * sign[None, :]
        weights = (ours.components_ / (np.sqrt(ours.explained_variance_)[:, None] if whiten else 1.0)).T.astype(np.float32)
        _, bound = PC.projection_bound(x, 12, ours.mean_.astype(np.float32), weights)
        # + the two models' own difference: a unit vector at sine s from another is within sqrt(2) s of it (Davis-Kahan
        # as in tests/pca_cases.py), and |d . dv| <= |d| |dv|; whitening divides by a standard deviation that is itself
        # within d_c / (2 value) relative; + one float32 rounding of the weights (inside the bound's spare u)
        for j in range(5):
            gap = np.abs(np.delete(values, j) - values[j]).min()
            turn = np.sqrt(2) * (2 * d_c / gap + 1e-7) + (d_c / values[j] if whiten else 0.0)
            scale = 1.0 / np.sqrt(values[j]) if whiten else 1.0
            slack = bound[:, j] + np.linalg.norm(x64 - x64.mean(0), axis=1) * turn * scale + 1e-9
            assert (np.abs(got[:, j] - want[:, j]) <= slack).all(), (whiten, j)


def outputs(directory):
    return {name: open(os.path.join(directory, name), "rb").read() for name in sorted(os.listdir(directory))}


@pytest.mark.parametrize("estimator", T.ESTIMATORS)
def test_trainer_with_each_estimator(estimator, tmp_path):
    be = EmuBackend()
    log, out = tmp_path / "log", tmp_path / "out"
    result = T.main(["--estimator", estimator, "--forest_trees", "4", "--pca_components", "3", "--fullscene",
                     "--base_log_path", str(log), "--output_path", str(out)] + COMMON, backend=be)
    est, predicted, cm, _, scene = result[0]
    features = est.n_features_in_ if hasattr(est, "n_features_in_") else est._f
    assert features == 5 * 5 * (3 + 1)
    assert scene.shape == (20, 24) and cm.sum() == len(predicted)
    assert {"pca_band_sums_f64", "pca_scatter_f64", "pca_project_f32"} <= set(be.launch_log)
    assert be.launch_log.count("pca_band_sums_f64") == 1 and be.launch_log.count("pca_scatter_f64") == 1
    assert be.launch_log.count("pca_project_f32") == 3  # training rows, validation rows, the scene
    report = json.load(open(log / "pca_SyntheticDataLoader.json"))
    assert set(report) == {"n_components", "n_samples", "bands", "whiten", "explained_variance", "explained_variance_ratio"}
    assert (report["n_components"], report["n_samples"], report["bands"], report["whiten"]) == (3, 480, 8, False)
    assert len(report["explained_variance"]) == len(report["explained_variance_ratio"]) == 3
    arrays = np.load(log / "pca_SyntheticDataLoader.npz")
    assert set(arrays.files) == {"mean_", "components_", "explained_variance_"}
    assert arrays["components_"].shape == (3, 8) and arrays["mean_"].shape == (8,)
    assert np.array_equal(arrays["explained_variance_"], np.array(report["explained_variance"]))
    assert os.path.exists(out / "result_raw.tif") and os.path.exists(log / "metrics_SyntheticDataLoader_run0.txt")


def test_trainer_fraction_whitening_and_forest_diagnostics(tmp_path):
    be = EmuBackend()
    result = T.main(["--estimator", "forest", "--forest_trees", "4", "--pca_components", "0.999", "--pca_whiten",
                     "--forest_importances", "--split_count", "2", "--base_log_path", str(tmp_path)] + COMMON, backend=be)
    report = json.load(open(tmp_path / "pca_SyntheticDataLoader.json"))
    k = report["n_components"]
    assert report["whiten"] is True and 1 <= k < 8 and sum(report["explained_variance_ratio"]) > 0.999
    assert be.launch_log.count("pca_scatter_f64") == 1  # fitted once per process, not per episode
    assert result[0][0].n_features_in_ == 25 * (k + 1)
    # the band axis of the diagnostics means components (+ the LiDAR channel)
    assert np.load(tmp_path / "feature_importance_SyntheticDataLoader_run1.npy").shape == (5, 5, k + 1)
    assert len(open(tmp_path / "band_importance_SyntheticDataLoader_run0.csv").read().splitlines()) == 1 + k + 1
    for bad in ("-1", "1.5", "1.0", "x"):
        with pytest.raises(SystemExit):
            T.main(["--pca_components", bad] + COMMON, backend=EmuBackend())


def test_trainer_with_zero_components_is_the_trainer_without_the_flag(tmp_path, capsys):
    runs = {}
    for name, extra in (("without", []), ("zero", ["--pca_components", "0"])):
        be = EmuBackend()
        capsys.readouterr()
        T.main(["--estimator", "forest", "--forest_trees", "4", "--fullscene", "--base_log_path", str(tmp_path / name / "log"),
                "--output_path", str(tmp_path / name / "out")] + extra + COMMON, backend=be)
        printed = [line for line in capsys.readouterr().out.splitlines() if "sec)" not in line]  # (wall-clock lines)
        runs[name] = (be.launch_log, outputs(tmp_path / name / "log"), outputs(tmp_path / name / "out"), printed)
    assert runs["zero"] == runs["without"]
    assert not any(entry.startswith("pca_") for entry in runs["zero"][0])
    assert not any(name.startswith("pca_") for name in runs["zero"][1])
