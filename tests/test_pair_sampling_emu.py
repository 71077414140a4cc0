"""CPU: the shadow / lit pairing against the pairs the reference's own samplers produced on the same seeded scenes
(tests/golden/reference_pair_sampling.*, written by tests/golden/make_reference_pair_sampling.py) -- the host samplers,
and the device path of gan_sampling_methods on the NumPy emulation of the pairing launches (tests/emu_pairs.py).  All
comparisons are exact: this is data movement."""
import json
import os

import numpy as np
import pytest
import torch

import tests.emu_pairs as E  # registers the pairing launches on EmuBackend
from hypelcnn_amd.backend import Ref
from hypelcnn_amd.gan import gan_sampling_methods as S
from hypelcnn_amd.gan.gan_train_for_shadow import PairIterator, read_hsi_data
from tests import pair_cases as C
from tests.emu_backend import EmuBackend

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    meta = json.load(open(os.path.join(GOLDEN, "reference_pair_sampling.json")))
    with np.load(os.path.join(GOLDEN, "reference_pair_sampling.npz")) as z:
        return meta, {k: z[k] for k in z.files}


def scene_of(gold, name):
    meta, arrays = gold
    s = {k: arrays.get(f"scene/{name}/{k}") for k in ("casi", "lidar", "map", "targets")}
    s.update(meta["scenes"][name])
    return s


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fixture_scenes_are_the_builders(gold):
    for name in C.SCENES:
        built, kept = C.build_scene(name), scene_of(gold, name)
        for k in ("casi", "lidar", "map", "targets"):
            assert (built[k] is None and kept[k] is None) or np.array_equal(built[k], kept[k]), (name, k)


# ----------------------------------------------------------------------------- the emulation's dilation
MAPS = {"empty": lambda h, w, r: np.zeros((h, w), np.uint8), "full": lambda h, w, r: np.ones((h, w), np.uint8),
        "corners": None, "sparse": lambda h, w, r: (r.random((h, w)) < 0.05).astype(np.uint8)}


def make_map(kind, h, w, seed=0):
    if kind == "corners":
        m = np.zeros((h, w), np.uint8)
        m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1
        return m
    return MAPS[kind](h, w, np.random.default_rng(seed))


@pytest.mark.parametrize("radius", [1, 2, 20])
@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (5, 7), (23, 70), (70, 23), (130, 259)])
def test_emu_dilation_is_scipys(shape, radius):
    ndimage = pytest.importorskip("scipy.ndimage")
    for kind in MAPS:
        m = make_map(kind, *shape, seed=radius)
        want = ndimage.binary_dilation(m, iterations=radius).astype(np.uint8)
        assert np.array_equal(E.dilate_l1(m, radius), want), kind


# ----------------------------------------------------------------------------- the entry points on small tables
def test_emu_compaction_and_expansion():
    be = EmuBackend()
    rng = np.random.default_rng(3)
    mask = (rng.random((9, 13)) < 0.3).astype(np.uint8) * 7  # any non-zero value selects
    pts = S.device_compact(be, be.upload(mask), 9, 13).numpy()
    ys, xs = np.nonzero(mask)
    assert pts.dtype == np.int32 and np.array_equal(pts, np.stack([xs, ys], axis=1))
    src = np.arange(6, dtype=np.int32).reshape(3, 2)
    out = be.empty(2 * 14, torch.int32)
    be.call("points_expand_i32", Ref(be.upload(src)), 3, 4, 2, Ref(out))
    assert np.array_equal(out.numpy().reshape(14, 2), np.vstack([np.repeat(src, 4, axis=0), src[:2]]))
    assert np.array_equal(S.device_expand(be, torch.from_numpy(src), 2).numpy(), np.repeat(src, 2, axis=0))


# ----------------------------------------------------------------------------- samplers against the reference
@pytest.mark.parametrize("case", list(C.CASES))
def test_host_sampler_is_the_references(gold, case):
    meta, arrays = gold
    scene, cls, kwargs = C.CASES[case]
    assert meta["cases"][case] == {"scene": scene, "sampler": cls, "args": kwargs,
                                   "normal": list(arrays[f"case/{case}/normal"].shape),
                                   "shadow": list(arrays[f"case/{case}/shadow"].shape)}
    s = scene_of(gold, scene)
    data_set, loader = C.stubs(s)
    normal, shadow = getattr(S, cls)(**kwargs).get_sample_pairs(data_set, loader, s["map"])
    assert same_bits(normal, arrays[f"case/{case}/normal"])
    assert same_bits(shadow, arrays[f"case/{case}/shadow"])


@pytest.mark.parametrize("hsi_only", [False, True])
@pytest.mark.parametrize("case", list(C.CASES))
def test_device_path_on_the_emulation_is_the_references(gold, case, hsi_only):
    _, arrays = gold
    scene, cls, kwargs = C.CASES[case]
    s = scene_of(gold, scene)
    data_set, loader = C.stubs(s)
    be = EmuBackend()
    normal, shadow = getattr(S, cls)(**kwargs).get_sample_pairs_device(data_set, loader, s["map"], be, hsi_only=hsi_only)
    bands = s["casi"].shape[2] if hsi_only else None
    assert same_bits(normal.numpy(), arrays[f"case/{case}/normal"][..., :bands])
    assert same_bits(shadow.numpy(), arrays[f"case/{case}/shadow"][..., :bands])


def test_registry_samplers_offer_the_device_path():
    from hypelcnn_amd.gan.wrapper_registry import get_sampling_map
    m = get_sampling_map()
    assert all(hasattr(m[k], "get_sample_pairs_device") for k in ("neighbour", "random", "target"))
    assert not hasattr(m["dummy"], "get_sample_pairs_device")


# ----------------------------------------------------------------------------- read_hsi_data and the iterator
class EmuDeviceSet:
    """What read_hsi_data needs of a DeviceBasicDataSet, over the emulation: built without scene launches."""

    def __new__(cls, scene, backend):
        from hypelcnn_amd.common.device_scene import DeviceBasicDataSet
        ds = DeviceBasicDataSet.__new__(DeviceBasicDataSet)
        ds.backend, ds.neighborhood, ds._host = backend, scene["neighborhood"], {}
        ds.casi_dev = torch.from_numpy(scene["casi"])
        ds.lidar_dev = None if scene["lidar"] is None else torch.from_numpy(scene["lidar"])
        return ds


@pytest.mark.parametrize("method,case", [("neighbour", "neighbour_registry"), ("random", "random_multiplied")])
def test_read_hsi_data_takes_the_device_path(gold, method, case):
    from hypelcnn_amd.gan.wrapper_registry import get_sampling_map
    _, arrays = gold
    s = scene_of(gold, C.CASES[case][0])
    ds = EmuDeviceSet(s, EmuBackend())
    normal, shadow = read_hsi_data(C.stubs(s)[1], ds, s["map"], method, get_sampling_map())
    assert isinstance(normal, torch.Tensor) and isinstance(shadow, torch.Tensor)
    bands = s["casi"].shape[2]
    assert same_bits(normal.numpy(), arrays[f"case/{case}/normal"][..., :bands])
    assert same_bits(shadow.numpy(), arrays[f"case/{case}/shadow"][..., :bands])
    assert ds.downloaded() == []
    # a host data set, and the dummy sampler on a device one, stay on the host path
    host_n, host_s = read_hsi_data(C.stubs(s)[1], C.stubs(s)[0], s["map"], method, get_sampling_map())
    assert isinstance(host_n, np.ndarray) and same_bits(host_n, normal.numpy()) and same_bits(host_s, shadow.numpy())
    dummy_n, _ = read_hsi_data(C.stubs(s)[1], ds, s["map"], "dummy", get_sampling_map())
    assert isinstance(dummy_n, np.ndarray)


def test_pair_iterator_keeps_device_tensors():
    normal, shadow = torch.rand(10, 1, 1, 4), torch.rand(10, 1, 1, 4)
    it = PairIterator(normal, shadow, 4, 5, None, 0.0, torch.device("cpu"))
    assert it.normal.data_ptr() == normal.data_ptr() and it.shadow.data_ptr() == shadow.data_ptr()
    x, y = it.next_batch()
    assert x.shape == (4, 4) and y.shape == (4, 4)


# ----------------------------------------------------------------------------- refusals
def test_device_path_refusals(gold):
    s = scene_of(gold, "a")
    data_set, loader = C.stubs(s)
    be = EmuBackend()
    ring = S.NeighborhoodBasedSampler(neighborhood_size=5, margin=2)
    rand = S.RandomBasedSampler(multiply_shadowed_data=True)
    two = s["map"].copy()
    two[3, 3] = 2
    for sampler in (ring, rand, S.TargetBasedSampler(margin=2)):
        with pytest.raises(ValueError, match="other than 0 and 1"):
            sampler.get_sample_pairs_device(data_set, loader, two, be)
        with pytest.raises(ValueError, match="is not the scene's"):
            sampler.get_sample_pairs_device(data_set, loader, np.pad(s["map"], 1), be)
    for bad in (dict(neighborhood_size=5, margin=0), dict(neighborhood_size=0, margin=2)):
        with pytest.raises(ValueError, match="at least 1"):
            S.NeighborhoodBasedSampler(**bad).get_sample_pairs_device(data_set, loader, s["map"], be)
    for sampler in (ring, rand):
        with pytest.raises(ValueError, match="no shadowed pixel"):
            sampler.get_sample_pairs_device(data_set, loader, np.zeros_like(s["map"]), be)
    with pytest.raises(ValueError, match="no lit pixel"):
        rand.get_sample_pairs_device(data_set, loader, np.ones_like(s["map"]), be)
    with pytest.raises(ValueError, match="no lit pixel lies in the ring"):
        # margin == neighborhood_size: the ring is empty
        S.NeighborhoodBasedSampler(neighborhood_size=2, margin=2).get_sample_pairs_device(data_set, loader, s["map"], be)
    mostly = np.ones_like(s["map"])
    mostly[0, :3] = 0
    with pytest.raises(ValueError, match="fewer lit than shadowed"):
        rand.get_sample_pairs_device(data_set, loader, mostly, be)
    with pytest.raises(ValueError, match="no class has both"):
        S.TargetBasedSampler(margin=2).get_sample_pairs_device(data_set, loader, np.zeros_like(s["map"]), be)
