"""GPU: the band-PCA launches of csrc/pca.hip against float64 NumPy on the same float32 input, within the derived bounds
of tests/pca_cases.py (none is tuned) -- on data with band means of 2000 to 12000 over standard deviations from 30 down to
0.007 and one constant band, as a plain row matrix and as the interior of a padded scene whose origin is 4-byte aligned
only, every output between sentinel bytes, every launch twice with equal bits; BandPCA on the device against the float64
eigh; and classic_ml_trainer --pca_components on the device against the same run on the NumPy twin."""
import json

import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import PCA_CHUNK, PCA_MAX_BLOCKS, Ref
from hypelcnn_amd.classic.decomposition import BandPCA
from tests import pca_cases as PC

pytestmark = pytest.mark.gpu

PROJECT_BANDS = (1, 3, 17, 64, 65, 145, 512)  # below, at and past the 64-band chunk and the 64-column pass of the kernel
PROJECT_BLOCK_ROWS, PROJECT_MAX_BLOCKS = 64, 4096


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def fit_case(be, x):
    """every layout, each twice: equal bits between the runs and between the layouts, the bounds on each -> error shares"""
    worst = (0.0, 0.0)
    first = None
    for _, buf, origin, h, w, sy, sx in PC.layouts(x):
        got = PC.run_fit_launches(be, buf, origin, h, w, x.shape[1], sy, sx)
        again = PC.run_fit_launches(be, buf, origin, h, w, x.shape[1], sy, sx)
        for a, b in zip(got, again):
            assert np.array_equal(bits(a), bits(b))
        if first is None:
            first = got
        for a, b in zip(got, first):  # the chunks are cut by pixel index, not by address
            assert np.array_equal(bits(a), bits(b))
        shares = PC.check_fit_launches(x, *got)
        worst = (max(worst[0], shares[0]), max(worst[1], shares[1]))
    return worst


@pytest.mark.parametrize("c", PC.BANDS)
def test_sums_and_scatter(be, c):
    for n in PC.PIXELS:
        sums_share, scatter_share = fit_case(be, PC.hard_pixels(n, c))
        print(f"pca fit c={c} n={n}: sums error / bound {sums_share:.3g}, scatter error / bound {scatter_share:.3g}")


def test_sums_and_scatter_one_chunk_past_a_grid_pass(be):
    """3 bands: one scatter tile, so both fit kernels run HYPEL_PCA_MAX_BLOCKS blocks and block 0 takes a second chunk,
    of one pixel."""
    n = PCA_MAX_BLOCKS * PCA_CHUNK + 1
    sums_share, scatter_share = fit_case(be, PC.hard_pixels(n, 3))
    print(f"pca fit c=3 n={n}: sums error / bound {sums_share:.3g}, scatter error / bound {scatter_share:.3g}")


def project_case(be, x, c, pass_cols, k, spots, seed=0):
    """x: [n, c + pass_cols]; the rows `spots` hold one and the same pixel.  -> largest error / bound"""
    n = x.shape[0]
    rng = np.random.default_rng([seed, c, k, pass_cols])
    x = x.copy()
    x[spots] = x[spots[0]]
    ldx, ldo = c + pass_cols + 1, k + pass_cols + 3
    wide = np.full((n, ldx), np.nan, np.float32)  # the float between the rows is never read
    wide[:, :c + pass_cols] = x
    mean32 = x[:, :c].astype(np.float64).mean(0).astype(np.float32)
    weights = (rng.standard_normal((c, k)) / np.sqrt(c)).astype(np.float32)
    x_d, mean_d, weights_d = be.upload(wide), be.upload(mean32), be.upload(weights)
    runs = []
    for _ in range(2):
        out, intact = PC.guarded(be, n * ldo, np.float32)
        be.call("pca_project_f32", Ref(x_d), 1, n, c, n * ldx, ldx, pass_cols, Ref(mean_d), Ref(weights_d), k, Ref(out), ldo)
        runs.append(out.cpu().numpy().copy().reshape(n, ldo))
        assert intact()
    got = runs[0]
    assert np.array_equal(bits(runs[1]), bits(got))
    want, bound = PC.projection_bound(x, c, mean32, weights)
    err = np.abs(got[:, :k].astype(np.float64) - want)
    assert (err <= bound).all(), float((err / np.where(bound > 0, bound, 1)).max())
    assert np.array_equal(bits(got[:, k:k + pass_cols]), bits(x[:, c:]))          # passed through bit for bit
    assert (bits(got[:, k + pass_cols:]) == PC.SENTINEL).all()                    # beyond k + pass: untouched
    for spot in spots[1:]:                                                        # the same pixel, the same bits
        assert np.array_equal(bits(got[spot, :k + pass_cols]), bits(got[spots[0], :k + pass_cols])), spot
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0.0)))


@pytest.mark.parametrize("c", PROJECT_BANDS)
def test_projection(be, c):
    n = 2 * PROJECT_BLOCK_ROWS + 3  # two full blocks and a tail of three rows
    for pass_cols in (0, 1, 2):
        x = np.concatenate([PC.hard_pixels(n, c, seed=7), PC.hard_pixels(n, 2, seed=8)[:, :pass_cols]], axis=1)
        for k in sorted({1, min(7, c), c}):
            share = project_case(be, x, c, pass_cols, k, [0, PROJECT_BLOCK_ROWS - 1, n - 1])
            print(f"pca project c={c} k={k} pass={pass_cols}: error / bound {share:.3g}")


def test_projection_one_row_past_a_grid_pass(be):
    n = PROJECT_MAX_BLOCKS * PROJECT_BLOCK_ROWS + 1
    x = np.concatenate([PC.hard_pixels(n, 3, seed=9), PC.hard_pixels(n, 2, seed=10)[:, :1]], axis=1)
    share = project_case(be, x, 3, 1, 2, [0, n - 2, n - 1])
    print(f"pca project c=3 k=2 pass=1 n={n}: error / bound {share:.3g}")


def test_band_pca_against_the_float64_eigh(be):
    x = PC.spectrum_pixels(5000, 12)
    pca = BandPCA(6, backend=be).fit(x)
    value_share, sine_share = PC.check_against_eigh(pca, x)
    print(f"BandPCA 12 bands, 5000 pixels: eigenvalue error / bound {value_share:.3g}, sine / bound {sine_share:.3g}")
    # the same pixels as a strided view of a device tensor: the interior of a padded raster
    scene = torch.full((54, 104, 13), float("nan"), device=be.device)
    scene[2:52, 2:102, :12] = torch.from_numpy(x.reshape(50, 100, 12)).to(be.device)
    on_view = BandPCA(6, backend=be).fit(scene[2:52, 2:102, :12])
    for name in ("mean_", "components_", "explained_variance_"):
        assert np.array_equal(bits(getattr(on_view, name)), bits(getattr(pca, name))), name
    hard = PC.hard_pixels(3000, 17, seed=3)
    full = BandPCA(17, backend=be).fit(hard)
    values = np.linalg.eigvalsh(np.cov(hard.astype(np.float64).T))[::-1]
    assert (np.abs(full.explained_variance_ - np.clip(values, 0, None)) <= PC.covariance_bound(hard, full.mean_, values[0])).all()


@pytest.mark.parametrize("path", ["grss2013:bands=8:classes=4:h=20:w=24", "grss2013:bands=8:classes=4:h=20:w=24:lidar=0",
                                  "grss2018hr:bands=8:classes=4:h=20:w=24"])
def test_rows_cut_from_the_projected_scene_are_the_projected_rows(be, path):
    from tests.test_pca_emu import check_rows_cut_from_the_projected_scene
    check_rows_cut_from_the_projected_scene(be, path)


def test_trainer_on_the_device_agrees_with_the_emulation(be, tmp_path):
    """The twin's projection is NOT bit-compatible with the device's (tests/emu_pca.py: its fmaf is rounded twice, and its
    scatter is summed in NumPy's order), so the second form of the check applies: the validation predictions of the two
    runs agree on at least the share of rows that the derived projection bound cannot flip.

    How that share is derived.  Both runs write their fitted model (pca_<loader>.npz).  For a patch pixel with centred
    bands d the two float32 projections differ by at most |d (W_dev - W_emu) in float64, each about its own mean| + the
    projection bound of either side (tests/pca_cases.py); that is delta, per row and feature, the LiDAR channel
    (passed through bit for bit) has none.  The forests are grown from a host-side random stream on the ranks of the
    training values, so their thresholds are training values that moved by no more than the largest delta of their
    feature.  A validation row can then only change its path where a feature lies within its delta + that largest delta
    of a threshold the device forest uses on that feature (any node: the path is not followed).  Premise, not derived:
    no two training values of a feature swap ranks between the runs (that would regrow a tree)."""
    from hypelcnn_amd.classify import classic_ml_trainer as T
    from hypelcnn_amd.importer.InMemoryImporter import InMemoryImporter
    from tests import emu_forest, emu_pca, emu_scene  # noqa: F401 -- attach the emulations to EmuBackend
    from tests.emu_backend import EmuBackend
    path, k = "grss2013", 8
    runs = {}
    for name, backend in (("device", be), ("emulation", EmuBackend())):
        log = tmp_path / name
        out = T.main(["--estimator", "forest", "--forest_trees", "8", "--pca_components", str(k), "--fullscene",
                      "--loader_name", "SyntheticDataLoader", "--path", path, "--neighborhood", "2",
                      "--base_log_path", str(log), "--output_path", str(log)], backend=backend)
        est, predicted, _, (oa, _, _), scene = out[0]
        model = np.load(log / "pca_SyntheticDataLoader.npz")
        report = json.load(open(log / "pca_SyntheticDataLoader.json"))
        assert report["n_components"] == k and report["bands"] == 144 and report["n_samples"] == 60 * 80
        assert est.n_features_in_ == 25 * (k + 1) and scene.shape == (60, 80)
        runs[name] = (est, np.asarray(predicted), model["mean_"].astype(np.float32), model["components_"].T.astype(np.float32),
                      oa, scene)
    training, _, validation, _, _, _, _ = InMemoryImporter().read_data_set(
        loader_name="SyntheticDataLoader", path=path, test_data_ratio=0, train_data_ratio=0.1, neighborhood=2,
        normalize=False)

    def sides(patches):
        rows = np.ascontiguousarray(patches, dtype=np.float32).reshape(-1, 145)
        dev, dev_bound = PC.projection_bound(rows, 144, runs["device"][2], runs["device"][3])
        emu, emu_bound = PC.projection_bound(rows, 144, runs["emulation"][2], runs["emulation"][3])
        n = len(patches)
        pad = np.zeros((n * 25, 1))  # the LiDAR channel
        delta = np.concatenate([np.abs(dev - emu) + dev_bound + emu_bound, pad], axis=1).reshape(n, -1)
        return np.concatenate([dev, pad], axis=1).reshape(n, -1), np.concatenate([dev_bound, pad], axis=1).reshape(n, -1), delta

    _, _, train_delta = sides(training.data)
    features, own_bound, delta = sides(validation.data)
    reach = np.maximum(train_delta.max(0), delta.max(0))  # how far a threshold of a feature can have moved
    forest = runs["device"][0]
    can_flip = np.zeros(len(features), bool)
    for f in np.unique(forest.feature_[forest.feature_ >= 0]):
        cuts = np.sort(forest.threshold_[forest.feature_ == f].astype(np.float64))
        at = np.searchsorted(cuts, features[:, f])
        nearest = np.minimum(np.abs(features[:, f] - cuts[np.clip(at - 1, 0, len(cuts) - 1)]),
                             np.abs(features[:, f] - cuts[np.clip(at, 0, len(cuts) - 1)]))
        can_flip |= nearest <= delta[:, f] + own_bound[:, f] + reach[f]
    share = 1.0 - can_flip.mean()
    agreement = float(np.mean(runs["device"][1] == runs["emulation"][1]))
    scene_agreement = float(np.mean(runs["device"][5] == runs["emulation"][5]))
    print(f"trainer --pca_components {k}: validation rows that cannot flip {share:.4f}, agreement {agreement:.4f}, "
          f"scene agreement {scene_agreement:.4f}, OA device {runs['device'][4]:.4f} emulation {runs['emulation'][4]:.4f}")
    assert agreement >= share
