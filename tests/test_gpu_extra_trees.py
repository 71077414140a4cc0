"""-m gpu: hypelcnn_amd.classic.forest.ExtraTreesForest on the device, held BIT FOR BIT to the numpy emulation of the
same entry points (tests/emu_forest.py) running the same host code with the same seeded stream: the feature-major
copy, every level's (score, thr, valid) table, the grown node arrays, labels, probabilities and scene rasters.  Eight
trees per case."""
import numpy as np
import pytest
import torch

from hypelcnn_amd.classic import forest as P
from tests import emu_forest, emu_scene  # noqa: F401 -- attach the emulations to EmuBackend
from tests import extra_trees_cases as XC
from tests import forest_cases as FC
from tests.emu_backend import EmuBackend

pytestmark = pytest.mark.gpu
CASES = ["small", "grss2013"]


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


_pairs = {}


def make(case, be):
    return XC.recording_extra_trees()(backend=be, **FC.CASES[case][1])


def pair(case, hip):
    """(the emulation's trees, the device's) of a case, fitted once"""
    if case not in _pairs:
        X, y, _, _ = FC.load(case)
        _pairs[case] = tuple(make(case, be).fit(X, y) for be in (EmuBackend(), hip))
    return _pairs[case]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", CASES)
def test_columns_and_every_level_table(case, hip):
    emu, dev = pair(case, hip)
    assert emu._ldn == dev._ldn and same(emu._xt.numpy(), dev._xt.cpu().numpy())
    assert emu.n_levels_ == dev.n_levels_ == len(emu.level_records_) == len(dev.level_records_)
    for level, (a, b) in enumerate(zip(emu.level_records_, dev.level_records_)):
        for name, u, v in zip(("active", "cand", "score", "thr", "valid"), a, b):
            assert same(u, v), (level, name)
    assert emu.level_records_[0][4].any()
    counts = np.concatenate([rec[0][:, 2] for rec in emu.level_records_])
    assert counts.max() > 64 and (counts <= 64).any()  # nodes on either side of one wavefront's rows


@pytest.mark.parametrize("case", CASES)
def test_grown_trees(case, hip):
    emu, dev = pair(case, hip)
    XC.same_arrays(emu.arrays(), dev.arrays(), case)
    for k in ("leaf_", "leaf_value_", "threshold_bin_", "node_count_", "node_weight_"):
        assert same(getattr(emu, k), getattr(dev, k)), k
    assert (dev.threshold_bin_ == -1).all()
    print(case, len(emu.feature_), "nodes,", emu.n_levels_, "levels")


def test_two_fits_write_identical_bytes(hip):
    X, y, _, _ = FC.load("small")
    _, first = pair("small", hip)
    again = make("small", hip).fit(X, y)
    XC.same_arrays(first.arrays(), again.arrays(), "second fit")
    for a, b in zip(first.level_records_, again.level_records_):
        assert all(same(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("case", CASES)
def test_training_rows_come_back(case, hip):
    """purity on the device: no bootstrap, no depth cap met, so every leaf holds one class"""
    _, dev = pair(case, hip)
    X, y, _, _ = FC.load(case)
    assert dev.n_levels_ <= P.FOREST_MAX_DEPTH and not dev.bootstrap
    assert np.array_equal(dev.predict(X), y)
    leaves = dev.value_[dev.left_ < 0]
    assert ((leaves == 0) | (leaves == 1)).all() and (leaves.sum(1) == 1).all()


@pytest.mark.parametrize("case", CASES)
def test_predict_and_proba(case, hip):
    emu, dev = pair(case, hip)
    X, _, Xv, _ = FC.load(case)
    rows = np.concatenate([Xv, X[:301]])  # more than one block, not a multiple of the block
    assert same(emu.predict(rows), dev.predict(rows))
    assert same(emu.predict_proba(rows), dev.predict_proba(rows))


@pytest.mark.parametrize("case", CASES)
def test_predict_scene_both_paths(case, hip):
    emu, dev = pair(case, hip)
    arrays_e, (h, w) = FC.scene_arrays(case, emu._backend())
    want = torch.zeros(h * w, dtype=torch.uint8)
    emu.predict_scene(arrays_e, want, w, direct=False)
    arrays_d, _ = FC.scene_arrays(case, hip)
    for direct in (True, False):
        raster = torch.zeros(h * w, dtype=torch.uint8, device=hip.device)
        dev.predict_scene(arrays_d, raster, w, direct=direct)
        assert same(raster.cpu().numpy(), want.numpy()), direct
    assert len(np.unique(want.numpy())) > 1
