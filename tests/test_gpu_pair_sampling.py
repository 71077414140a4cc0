"""GPU: the pixel-pairing launches of csrc/pairs.hip against their NumPy twins (tests/emu_pairs.py) and the committed
pairs of the reference's samplers (tests/golden/reference_pair_sampling.*), and the device path of the samplers against
the host path on the host copy of the same device-prepared scene.  Everything is compared exactly."""
import json
import os

import numpy as np
import pytest
import torch

import tests.emu_pairs as E
from hypelcnn_amd.backend import COMPACT_TILE, Ref
from hypelcnn_amd.gan import gan_sampling_methods as S
from tests import pair_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def gold():
    meta = json.load(open(os.path.join(GOLDEN, "reference_pair_sampling.json")))
    with np.load(os.path.join(GOLDEN, "reference_pair_sampling.npz")) as z:
        return meta, {k: z[k] for k in z.files}


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ----------------------------------------------------------------------------- dilation
def contents(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    maps = {"empty": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8),  # any non-zero value is set
            "sparse": (rng.random((h, w)) < 0.05).astype(np.uint8)}
    for name, (y, x) in {"top_left": (0, 0), "top_right": (0, w - 1), "bottom_left": (h - 1, 0),
                         "bottom_right": (h - 1, w - 1)}.items():
        maps[name] = np.zeros((h, w), np.uint8)
        maps[name][y, x] = 1
    return maps


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (5, 7), (23, 70), (70, 23), (130, 259)])
def test_dilation(be, shape):
    h, w = shape
    for name, m in contents(h, w).items():
        map_d = be.upload(m)
        for radius in (1, 2, 20):
            got = S.device_dilate(be, map_d, h, w, radius).cpu().numpy().reshape(h, w)
            assert np.array_equal(got, E.dilate_l1(m, radius)), (name, radius)


def test_selection_masks(be):
    rng = np.random.default_rng(5)
    n = 3 * COMPACT_TILE + 77
    m = rng.integers(0, 2, n).astype(np.uint8)
    reach, margin = rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)
    map_d = be.upload(m)
    shadow, lit = S.device_pair_masks(be, map_d, n)
    assert np.array_equal(shadow.cpu().numpy(), m == 1) and np.array_equal(lit.cpu().numpy(), m != 1)
    shadow, lit = S.device_pair_masks(be, map_d, n, be.upload(reach), be.upload(margin))
    assert np.array_equal(shadow.cpu().numpy(), m == 1)
    assert np.array_equal(lit.cpu().numpy(), (reach != 0) & (margin == 0) & (m != 1))


# ----------------------------------------------------------------------------- compaction
def compact_raw(be, mask, h, w):
    """one call on zeroed buffers: (points bytes of the whole [h * w, 2] buffer, count)"""
    n = h * w
    points, count = be.zeros(2 * n, torch.int32), be.zeros(1, torch.int32)
    ws = be.zeros((n + COMPACT_TILE - 1) // COMPACT_TILE, torch.int32)
    be.call("mask_compact_points_i32", Ref(be.upload(mask)), h, w, Ref(points), n, Ref(count), Ref(ws))
    return points.cpu().numpy().reshape(n, 2), int(count.cpu()[0])


BIG = (1, 256 * COMPACT_TILE + 1)  # 257 tiles: the one-block scan over the tile counts takes a second trip


@pytest.mark.parametrize("shape", [(1, 1), (1, 255), (1, 256), (1, 257), (1, 65537), (130, 259), BIG])
def test_compaction(be, shape):
    h, w = shape
    n = h * w
    rng = np.random.default_rng(n)
    one = np.zeros((h, w), np.uint8)
    one[h - 1, w - 1] = 3
    masks = {"none": np.zeros((h, w), np.uint8), "one": one, "all": np.ones((h, w), np.uint8),
             "random": (rng.random((h, w)) < 0.4).astype(np.uint8)}
    if shape in ((130, 259), BIG):
        masks = {"all": masks["all"], "random": masks["random"]}
    for name, mask in masks.items():
        ys, xs = np.nonzero(mask)
        want = np.zeros((n, 2), np.int32)
        want[:ys.size] = np.stack([xs, ys], axis=1)
        points, count = compact_raw(be, mask, h, w)
        assert count == ys.size, name
        assert np.array_equal(points, want), name  # in order; rows past the count stay untouched
        again, count2 = compact_raw(be, mask, h, w)
        assert count2 == count and points.tobytes() == again.tobytes(), name


def test_compaction_respects_the_capacity(be):
    mask = np.ones((3, 50), np.uint8)
    points, count = be.zeros(2 * 150, torch.int32), be.zeros(1, torch.int32)
    be.call("mask_compact_points_i32", Ref(be.upload(mask)), 3, 50, Ref(points), 40, Ref(count), Ref(be.zeros(1, torch.int32)))
    got = points.cpu().numpy().reshape(150, 2)
    assert int(count.cpu()[0]) == 150 and not got[40:].any()
    assert np.array_equal(got[:40], np.stack([np.arange(40) % 50, np.arange(40) // 50], axis=1))


# ----------------------------------------------------------------------------- expansion
@pytest.mark.parametrize("n,repeat,remainder", [(1, 1, 0), (3, 4, 2), (257, 1, 256), (64, 5, 0)])
def test_expansion(be, n, repeat, remainder):
    src = np.random.default_rng(n).integers(0, 1 << 20, (n, 2)).astype(np.int32)
    got = S.device_expand(be, be.upload(src).reshape(n, 2), repeat, remainder).cpu().numpy()
    assert np.array_equal(got, np.vstack([np.repeat(src, repeat, axis=0), src[0:remainder]]))


# ----------------------------------------------------------------------------- samplers on the reference's fixture
@pytest.mark.parametrize("case", list(C.CASES))
def test_device_path_is_the_references(be, gold, case):
    meta, arrays = gold
    scene, cls, kwargs = C.CASES[case]
    s = {k: arrays.get(f"scene/{scene}/{k}") for k in ("casi", "lidar", "map", "targets")}
    s.update(meta["scenes"][scene])
    data_set, loader = C.stubs(s)
    normal, shadow = getattr(S, cls)(**kwargs).get_sample_pairs_device(data_set, loader, s["map"], be)
    assert normal.is_cuda and shadow.is_cuda
    assert same_bits(normal.cpu().numpy(), arrays[f"case/{case}/normal"])
    assert same_bits(shadow.cpu().numpy(), arrays[f"case/{case}/shadow"])


# ----------------------------------------------------------------------------- end to end on a device-prepared scene
def device_scene(be, path, neighborhood):
    """(loader, DeviceBasicDataSet of its scene, unpadded shadow map, host twin over the downloaded COPY of the scene)"""
    from hypelcnn_amd.common.device_scene import DeviceBasicDataSet
    from hypelcnn_amd.loader.SyntheticDataLoader import SyntheticDataLoader
    loader = SyntheticDataLoader(path)
    casi, lidar, _ = loader._scene()
    ds = DeviceBasicDataSet(None, casi, lidar, neighborhood, True, backend=be)
    twin = C.StubDataSet(ds.casi_dev.cpu().numpy(), None if ds.lidar_dev is None else ds.lidar_dev.cpu().numpy(),
                         neighborhood)
    return loader, ds, loader._shadow_map, twin


@pytest.mark.parametrize("path,neighborhood", [("avon:h=40:w=60:bands=12:classes=3", 0),
                                               ("grss2013:h=40:w=60:bands=12:classes=3", 0),
                                               ("grss2013:h=41:w=59:bands=5:classes=3", 2)])
@pytest.mark.parametrize("method", ["neighbour", "random", "target"])
def test_device_pairs_are_the_host_pairs(be, path, neighborhood, method):
    from hypelcnn_amd.gan.gan_train_for_shadow import read_hsi_data
    from hypelcnn_amd.gan.wrapper_registry import get_sampling_map
    loader, ds, smap, twin = device_scene(be, path, neighborhood)
    sampler = get_sampling_map()[method]
    want_n, want_s = sampler.get_sample_pairs(twin, loader, smap)
    assert want_n.shape[0] > 0 and want_n.shape == want_s.shape
    got_n, got_s = sampler.get_sample_pairs_device(ds, loader, smap, be)
    assert same_bits(got_n.cpu().numpy(), want_n) and same_bits(got_s.cpu().numpy(), want_s)
    # the trainer's entry: the casi bands alone, as device tensors, and nothing came back to the host
    hsi_n, hsi_s = read_hsi_data(loader, ds, smap, method, get_sampling_map())
    bands = ds.get_casi_band_count()
    assert hsi_n.is_cuda and hsi_s.is_cuda
    assert same_bits(hsi_n.cpu().numpy(), want_n[..., :bands]) and same_bits(hsi_s.cpu().numpy(), want_s[..., :bands])
    assert ds.downloaded() == []


def test_run_session_pairs_on_the_device(be, tmp_path, monkeypatch):
    from hypelcnn_amd.gan import gan_train_for_shadow as GT
    seen = {}
    real = GT.read_hsi_data

    def spy(loader, data_set, *args, **kwargs):
        out = real(loader, data_set, *args, **kwargs)
        seen["set"], seen["pairs"] = data_set, out
        return out

    monkeypatch.setattr(GT, "read_hsi_data", spy)
    flags, _ = GT.build_parser().parse_known_args(
        ["--loader_name", "SyntheticDataLoader", "--path", "avon:h=40:w=60:bands=16:device=1", "--gan_type", "cycle_gan",
         "--batch_size", "32", "--step", "2", "--pairing_method", "neighbour", "--base_log_path", str(tmp_path / "gan"),
         "--validation_sample_count", "64"])
    div = GT.run_session(dict(vars(flags)), flags.base_log_path)
    assert len(div) == 2 and all(np.isfinite(v) for v in div)
    assert type(seen["set"]).__name__ == "DeviceBasicDataSet" and seen["set"].downloaded() == []
    assert all(t.is_cuda for t in seen["pairs"])
