"""GPU: the file-backed loaders with the scene prepared on the device -- batches cut by SceneArrays from the resident
scene are the reference's patches bit for bit without the scene ever coming back to the host, MIXED batches follow the
member drawn per sample, and the classifier trains from the generated GRSS2013 directory."""
import json
import os

import numpy as np
import pytest
import torch

from hypelcnn_amd.common.common_nn_ops import SceneArrays, get_loader_from_name
from hypelcnn_amd.loader.DataLoader import LoadingMode
from tests import loader_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "reference_loaders.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return C.write_data_dir(str(tmp_path_factory.mktemp("loader_data")))


TARGETS = np.asarray([(x, y, 0) for x, y in C.POINTS])


@pytest.mark.parametrize("name,case,attrs", [
    ("GRSS2013DataLoader", "normalized", {}), ("GULFPORTDataLoader", "normalized", {}),
    ("GULFPORTALTDataLoader", "shadowed", {"_load_mode": LoadingMode.SHADOWED}),
    ("AVONDataLoader", "normalized", {}), ("AVONDataLoader", "shcorrected", {"load_shadow_corrected": True})])
def test_batches_from_the_resident_scene(be, gold, base, name, case, attrs):
    loader = get_loader_from_name(name, base)  # no backend given: the visible HIP device is used
    for k, v in attrs.items():
        setattr(loader, k, v)
    ds = loader.load_data(C.NEIGHBORHOOD, True)
    assert type(ds).__name__ == "DeviceBasicDataSet" and ds.casi_dev.is_cuda
    key = f"{name}/{case}"
    for what in ("casi_min", "casi_max", "lidar_min", "lidar_max"):
        got, want = np.asarray(getattr(ds, what)), gold[f"{key}/{what}"]
        assert got.dtype == want.dtype and np.array_equal(got, want), what
    if f"{key}/clip_bounds" in gold:
        assert np.array_equal(ds.clip_bounds, gold[f"{key}/clip_bounds"])
    arrays = SceneArrays()
    arrays.feed(ds, TARGETS, be)
    out, pts = arrays.gather(torch.arange(len(TARGETS), device=be.device))
    want = gold[f"{key}/patches"].astype(np.float32)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if f"{key}/shadow_ratio" in gold:
        ratio = np.asarray(ds.shadow_creator_dict["simple"].ratio)[:ds.get_casi_band_count()]
        ref = gold[f"{key}/shadow_ratio"].astype(np.float64)
        # the reference sums in float32 (n <= 1200 values per band: relative error <= n * 2^-24 on positive data)
        assert np.all(np.abs(ratio - ref) <= 2 * 1200 * 2.0 ** -24 * np.abs(ref))
    assert ds.downloaded() == [], "nothing on this path reads .casi / .lidar"


def test_mixed_batches_member_by_member(be, gold, base):
    loader = get_loader_from_name("GULFPORTALTDataLoader", base)
    loader._load_mode = LoadingMode.MIXED
    ds = loader.load_data(C.NEIGHBORHOOD, True)
    targets = np.tile(TARGETS, (4, 1))
    arrays = SceneArrays()
    arrays.feed(ds, targets, be)
    assert len(arrays.scenes) == 2
    out, _ = arrays.gather(torch.arange(len(targets), device=be.device))
    out = out.cpu().numpy()
    assert set(arrays.last_members) == {0, 1, 2, 3}
    for i, member in enumerate(arrays.last_members):
        want = gold[f"GULFPORTALTDataLoader/mixed/member{member}/patches"][i % len(TARGETS)].astype(np.float32)
        assert np.array_equal(out[i].view(np.uint32), want.view(np.uint32)), i
    assert all(m.downloaded() == [] for m in ds._data_sets)


def test_train_for_classification_from_grss2013_files(base, tmp_path):
    from hypelcnn_amd.classify import train_for_classification as T
    alg = {"batch_size": 32, "drop_out_ratio": 0.3, "filter_count": 32, "learning_rate": 3e-3,
           "learning_rate_decay_factor": 0.96, "learning_rate_decay_step": 350, "lrelu_alpha": 0.18,
           "optimizer": "AdamOptimizer", "bn_decay": 0.9, "l2regularizer_scale": 1e-5, "spectral_hierarchy_level": 1,
           "spatial_hierarchy_level": 1, "degradation_coeff": 3, "use_residual": True}
    p = tmp_path / "alg.json"
    p.write_text(json.dumps(alg))
    argv = ["--loader_name", "GRSS2013DataLoader", "--path", base, "--neighborhood", str(C.NEIGHBORHOOD),
            "--model_name", "HYPELCNNModel", "--algorithm_param_path", str(p), "--batch_size", "32", "--step", "3",
            "--base_log_path", str(tmp_path / "log")]
    flags, _ = T.build_parser().parse_known_args(argv)
    res = T.perform_an_episode(flags, dict(alg), T.get_model_from_name(flags.model_name),
                               os.path.join(flags.base_log_path, "run"))
    assert np.isfinite(res.loss)
