"""GPU: the scene-preparation launches of csrc/scene.hip and the shadow correction of csrc/components.hip over every
stored order, every extent-1 combination and the strides only as_strided can make (tests/scene_layout_cases.py): all
four (y_fast, band_fast) fetch paths of make_geom at more than one band, both sides of its tie rule, zero strides,
workspace slice counts from 1 to 1024 in workspaces exactly as long as the header asks, every output between sentinel
bytes, every launch twice with equal bits -- and everything against NumPy's own arithmetic on the view, bit for bit.
Then DeviceBasicDataSet on the six windowed views against the host BasicDataSet on a contiguous copy."""
import numpy as np
import pytest

from hypelcnn_amd.common import device_scene
from hypelcnn_amd.common.common_nn_ops import BasicDataSet
from tests import scene_layout_cases as L

pytestmark = pytest.mark.gpu

by_name = pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: np.dtype(d).name)


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@by_name
def test_extrema(be, dtype):
    for v in L.views(dtype):
        L.run_extrema(be, v, runs=2)


def test_rank_select(be):
    for v in L.views(np.uint16):
        L.run_rank_select(be, v, runs=2)


@by_name
def test_prepare(be, dtype):
    for v in L.views(dtype):
        L.run_prepare(be, v, runs=2)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_shadow_correct(be, dtype):
    for v in L.views(dtype):
        L.run_shadow_correct(be, v, runs=2)


def test_masked_sums(be):
    L.run_masked_sums(be, runs=2)


def host_data_set(monkeypatch, **kwargs):
    """make_basic_data_set's branch for a machine without a device: numpy.percentile, numpy.clip, BasicDataSet"""
    with monkeypatch.context() as m:
        m.setattr(device_scene, "resolve_scene_backend", lambda backend=None: None)
        return device_scene.make_basic_data_set(None, **kwargs)


@pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")
@pytest.mark.parametrize("kind", ["uint16", "float32", "uint16_clip95"])
def test_device_data_set_reads_every_stored_order(be, monkeypatch, kind):
    dtype = np.dtype(kind.split("_")[0])
    clip = 95 if kind.endswith("clip95") else None
    lidars = L.window_views(np.float32, (L.FULL[0], L.FULL[1], 1))
    host = None
    for v, lidar in zip(L.window_views(dtype), lidars):
        if host is None:  # the six views hold one scene: one host data set
            host = host_data_set(monkeypatch, shadow_creator_dict=None, casi=np.ascontiguousarray(v.view),
                                 lidar=np.ascontiguousarray(lidar.view), neighborhood=5, normalize=True,
                                 **({} if clip is None else {"clip_percentile": clip}))
            assert type(host) is BasicDataSet and host.casi.dtype == np.float32
        dev = device_scene.DeviceBasicDataSet(None, v.view, lidar.view, 5, True, backend=be, clip_percentile=clip)
        assert L.same_bits(dev.casi_dev.cpu().numpy(), host.casi), v
        assert L.same_bits(np.asarray(dev.casi_min), np.asarray(host.casi_min)), v
        assert L.same_bits(np.asarray(dev.casi_max), np.asarray(host.casi_max)), v
        assert L.same_bits(dev.lidar_dev.cpu().numpy(), host.lidar), v
        assert L.same_bits(np.asarray(dev.lidar_min), np.asarray(host.lidar_min)), v
        assert L.same_bits(np.asarray(dev.lidar_max), np.asarray(host.lidar_max)), v
        if clip is not None:
            assert L.same_bits(dev.clip_bounds, host.clip_bounds), v
            assert (host.clip_bounds < v.view.max(axis=(0, 1))).all()  # the clip does clip
