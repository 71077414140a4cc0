"""-m gpu: the random-forest kernels (csrc/forest.hip) and hypelcnn_amd.classic.forest on the device, held BIT FOR BIT to
the numpy emulation of the same entry points (tests/emu_forest.py) running the same host code with the same seeded
stream: edges, bins, the per-level score tables, the grown node arrays, labels, probabilities and scene rasters.  A
scikit-learn forest from tests/golden/reference_forest.npz, served on the device, gives scikit-learn's labels."""
import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import FOREST_EDGE_ROWS, FOREST_MAX_EDGES, Ref
from hypelcnn_amd.classic import forest as P
from tests import emu_forest, emu_scene  # noqa: F401 -- attach the emulations to EmuBackend
from tests import forest_cases as FC
from tests import svm_cases as S
from tests.emu_backend import EmuBackend

pytestmark = pytest.mark.gpu
CASES = ["small", "small_edges", "grss2013"]
LEVELS = 3


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def fixture():
    return FC.load_fixture()


_pairs = {}


def pair(case, hip):
    """(the emulation's forest, the device's) of a case, 8 trees, fitted once"""
    if case not in _pairs:
        X, y, _, _ = FC.load(case)
        models = []
        for be in (EmuBackend(), hip):
            m = FC.make(case, be)
            m.record_levels = LEVELS
            models.append(m.fit(X, y))
        _pairs[case] = tuple(models)
    return _pairs[case]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", CASES)
def test_edges_and_bins(case, hip):
    emu, dev = pair(case, hip)
    assert same(emu._n_edges.numpy(), dev._n_edges.cpu().numpy())
    assert same(emu._edges.numpy(), dev._edges.cpu().numpy())
    assert emu._ldn == dev._ldn and same(emu._bins.numpy(), dev._bins.cpu().numpy())
    ne = emu._n_edges.numpy()
    print(case, "edges per column", ne.min(), "..", ne.max())
    # the quantile path fills every slot; with fewer rows than bins no column can
    assert ne.max() == FOREST_MAX_EDGES if case == "grss2013" else ne.max() < 215


@pytest.mark.parametrize("n,f,n_bins", [(20000, 3, 256), (16384, 2, 256), (1, 2, 256), (777, 5, 16), (300, 4, 2)])
def test_bin_edges_sizes(hip, n, f, n_bins):
    """Past the row cap (a subsample through the permutation), exactly at it, one row, fewer bins; columns with
    duplicates, a constant one, signed zeros."""
    rng = np.random.default_rng(n + f)
    x = rng.standard_normal((n, f)).astype(np.float32)
    x[:, 0] = np.round(x[:, 0] * 2) / 2 * np.where(rng.random(n) < 0.5, -1, 1)  # few distinct values, -0.0 among them
    if f > 1:
        x[:, 1] = 3.25
    perm = rng.permutation(n).astype(np.int32)
    out = []
    for be in (EmuBackend(), hip):
        xd, pd = be.upload(x), be.upload(perm[:min(n, FOREST_EDGE_ROWS)])
        edges, ne = be.zeros(f * FOREST_MAX_EDGES), be.zeros(f, torch.int32)
        bins = be.zeros(f * (n + 3), torch.uint8)
        be.call("forest_bin_edges_f32", Ref(xd), f, n, f, Ref(pd), n_bins, Ref(edges), Ref(ne))
        be.call("forest_bin_u8", Ref(xd), f, n, f, Ref(edges), Ref(ne), Ref(bins), n + 3)
        be.synchronize()
        out.append([t.cpu().numpy() for t in (edges, ne, bins)])
    for a, b in zip(*out):
        assert same(a, b)
    assert out[0][1].max() <= n_bins - 1 and (f == 1 or out[0][1][1] == 0)


@pytest.mark.parametrize("case", CASES)
def test_first_levels_score_tables(case, hip):
    emu, dev = pair(case, hip)
    assert len(emu.level_records_) == len(dev.level_records_) == LEVELS
    for level, (a, b) in enumerate(zip(emu.level_records_, dev.level_records_)):
        for name, u, v in zip(("active", "cand", "score", "bin", "valid"), a, b):
            assert same(u, v), (level, name)
        assert a[4].any()


@pytest.mark.parametrize("case", CASES)
def test_grown_forest(case, hip):
    emu, dev = pair(case, hip)
    assert emu.n_levels_ == dev.n_levels_
    for k, v in emu.arrays().items():
        assert same(v, dev.arrays()[k]), k
    for k in ("leaf_", "leaf_value_", "threshold_bin_", "node_count_", "node_weight_"):
        assert same(getattr(emu, k), getattr(dev, k)), k
    print(case, len(emu.feature_), "nodes,", emu.n_levels_, "levels")


def test_two_fits_write_identical_bytes(hip):
    X, y, _, _ = FC.load("small")
    _, first = pair("small", hip)
    again = FC.make("small", hip).fit(X, y)
    for k, v in first.arrays().items():
        assert same(v, again.arrays()[k]), k
    assert same(first._bins.cpu().numpy(), again._bins.cpu().numpy())


@pytest.mark.parametrize("case", CASES)
def test_predict_and_proba(case, hip):
    emu, dev = pair(case, hip)
    X, _, Xv, yv = FC.load(case)
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


def test_chunked_serving_equals_one_launch(hip):
    """chunk_rows cuts the row kernel's work into launches that write at offsets into the same outputs."""
    _, dev = pair("small", hip)
    _, _, Xv, _ = FC.load("small")
    rows, (h, w) = S.load_scene_rows(FC.CASES["small"][0])
    arrays, _ = FC.scene_arrays("small", hip)
    want = dev.predict(rows), dev.predict_proba(Xv)
    try:
        dev.chunk_rows = 7  # 480 = 68 x 7 + 4, 24 = 3 x 7 + 3
        assert same(dev.predict(rows), want[0]) and same(dev.predict_proba(Xv), want[1])
        raster = torch.zeros(h * w, dtype=torch.uint8, device=hip.device)
        dev.predict_scene(arrays, raster, w, direct=False)
        assert same(raster.cpu().numpy(), want[0].astype(np.uint8))
    finally:
        dev.chunk_rows = None


@pytest.mark.parametrize("case", ["small", "grss2013"])
def test_served_scikit_learn_forest(case, hip, fixture):
    _, fx = fixture
    k = f"{case}/rf/"
    model = P.ForestClassifier.from_arrays(backend=hip, **FC.sk_arrays(fx, case))
    _, _, Xv, _ = FC.load(case)
    FC.check_served_labels(model.predict(Xv), fx[k + "proba_validation"], fx[k + "predict_validation"], case)
    assert np.array_equal(model.predict_proba(Xv), fx[k + "proba_validation"])  # the same fp64 sums in the same order
    if case == "small":
        rows, (h, w) = S.load_scene_rows(FC.CASES[case][0])
        FC.check_served_labels(model.predict(rows), fx[k + "proba_scene"], fx[k + "predict_scene"], case + "/scene")
        arrays, _ = FC.scene_arrays(case, hip)
        raster = torch.zeros(h * w, dtype=torch.uint8, device=hip.device)
        model.predict_scene(arrays, raster, w)
        FC.check_served_labels(raster.cpu().numpy(), fx[k + "proba_scene"], fx[k + "predict_scene"], case + "/raster")
