"""GPU: hypel_tensor_summary_f32 (csrc/summary.hip) against its twin (tests/emu_summary.py: numpy.searchsorted on the
limits table, math.fsum).  Bucket counts, min, max, num and the non-finite count are compared exactly; sum and
sum_squares must be within 64 * 2^-53 * sum|x| and 64 * 2^-53 * sum x^2 of math.fsum -- the bound of a pairwise or tree
fp64 sum of fewer than 2^64 terms; float32 values and their squares are exact in fp64, so nothing else contributes.
tests/summary_cases.check_against_twin prints every figure before it asserts."""
import math
import os

import numpy as np
import pytest

import tests.emu_summary as E
from hypelcnn_amd.backend import SUMMARY_SLICE
from hypelcnn_amd.common import tb_events
from tests import summary_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def shapes():
    return C.shape_case()


def test_boundaries(be):
    """the float32 neighbours of every finite non-zero limit (they straddle every boundary), +-0, the extreme
    subnormals, +-FLT_MIN, +-FLT_MAX: each lands in the bucket searchsorted gives"""
    values = C.boundary_values()
    assert values.size == 3096 + 10
    buf, segments, tensors = C.layout([values])
    got = C.launch(be, buf, segments)
    C.check_against_twin(got, tensors)
    assert got[2][0].max() <= 6 and got[0][0, 0] == -C.FLT_MAX and got[0][0, 1] == C.FLT_MAX


def test_another_limits_table(be):
    """the limits are data: a short table the logarithmic estimate knows nothing about is searched exactly too"""
    rng = np.random.default_rng(11)
    limits = np.asarray([-3.0, -0.1, 0.25, 0.5, 7.0, 1e30], np.float64)
    values = np.concatenate([(rng.standard_normal(5000) * 2).astype(np.float32), limits.astype(np.float32),
                             np.asarray([1e35, -1e35, 0.0], np.float32)])
    buf, segments, tensors = C.layout([values, values[:7]])
    C.check_against_twin(C.launch(be, buf, segments, limits), tensors, limits)


def test_segment_shapes_in_one_launch(be, shapes):
    """sizes 0, 1, 63, 64, 65, 4097, one slice, one slice + 1 and 3 * 2^20 + 5 (split over blocks) in ONE launch: odd
    element offsets (no 16-byte alignment), sentinel-filled gaps that must not be counted, table out of address order"""
    buf, segments, tensors = shapes
    assert {s for _, s in segments} >= {0, 1, 63, 64, 65, 4097, 3 * 2 ** 20 + 5}
    assert all(o % 2 == 1 for o, _ in segments) and [o for o, _ in segments] != sorted(o for o, _ in segments)
    got = C.launch(be, buf, segments)
    C.check_against_twin(got, tensors)
    sentinel_bucket = np.searchsorted(C.LIMITS, float(C.SENTINEL), side="right")
    assert got[2][:, sentinel_bucket].sum() == 0 and got[2].sum() == sum(t.size for t in tensors)


def test_contention(be):
    """2^22 copies of one value and 2^22 of two alternating values: all counts in one / two buckets, exactly"""
    n = 2 ** 22
    one = np.full(n, 0.0371, np.float32)
    two = np.tile(np.asarray([0.0371, -1.25], np.float32), n // 2)
    buf, segments, tensors = C.layout([one, two], odd_offsets=False)
    got = C.launch(be, buf, segments)
    C.check_against_twin(got, tensors)
    assert np.count_nonzero(got[2][0]) == 1 and got[2][0].max() == n
    assert np.count_nonzero(got[2][1]) == 2 and sorted(got[2][1][got[2][1] > 0]) == [n // 2, n // 2]


def test_non_finite(be):
    """NaN, +Inf and -Inf at block (slice) and wavefront boundaries of a 2^18 segment are counted and excluded; min and
    max are unaffected; an all-NaN segment gives num == 0 and the initial min and max"""
    rng = np.random.default_rng(13)
    n = 2 ** 18
    v = (rng.standard_normal(n) * 0.05).astype(np.float32)
    v[1000], v[2000] = -3.0, 4.0
    spots = [0, 1, 63, 64, 65, 255, 256, 1023, 1024, SUMMARY_SLICE - 1, SUMMARY_SLICE, SUMMARY_SLICE + 1,
             3 * SUMMARY_SLICE - 1, 3 * SUMMARY_SLICE, n - 65, n - 64, n - 1]
    for k, i in enumerate(spots):
        v[i] = (np.nan, np.inf, -np.inf)[k % 3]
    all_nan = np.full(300, np.nan, np.float32)
    buf, segments, tensors = C.layout([v, all_nan])
    got = C.launch(be, buf, segments)
    C.check_against_twin(got, tensors)
    stats, nonfinite, buckets = got
    assert nonfinite.tolist() == [len(spots), 300] and stats[0, :3].tolist() == [-3.0, 4.0, n - len(spots)]
    assert stats[1].tolist() == [E.DBL_MAX, -E.DBL_MAX, 0.0, 0.0, 0.0] and buckets[1].sum() == 0


def test_two_launches_give_identical_bits(be, shapes):
    buf, segments, _ = shapes
    a, b = C.launch(be, buf, segments), C.launch(be, buf, segments)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_slice_count_mismatch_is_refused(be):
    from hypelcnn_amd.common.device_summary import TensorSummary
    ts = TensorSummary(be, be.upload(np.ones(100, np.float32)), [(0, 50), (50, 50)], be.upload(C.LIMITS), C.LIMITS.size)
    ts.slices += 1
    ts.ws = be.zeros(ts.n + 1 + 6 * ts.slices, ts.ws.dtype)
    ts.launch()
    with pytest.raises(RuntimeError):
        ts.results()


def test_histograms_through_the_model(tmp_path, monkeypatch, capsys):
    """a few HYPELCNN steps at a small batch with --tensorboard_events --log_model_params: the event file passes every
    check of the emulated run, and the histograms of the last step -- the step the final checkpoint saves with
    sess.get_variable(name) -- equal the twin on those values"""
    from tests.test_summary_emu import check_events_of_run, run_episode
    log_dir = run_episode(tmp_path, None, ["--tensorboard_events", "true", "--log_model_params", "true"])
    histograms = check_events_of_run(log_dir, tmp_path, monkeypatch, capsys)
    last = max(histograms)
    with np.load(os.path.join(log_dir, f"model.ckpt-{last}.npz")) as z:
        assert len(histograms[last]) > 10
        for name, h in histograms[last].items():
            value = z[name.replace("/", "|")]
            stats, bad, counts = E.summarize(value, C.LIMITS)
            lim, cnt = tb_events.collapse_buckets(C.LIMITS, counts)
            assert bad == 0 and (h["min"], h["max"], h["num"]) == stats[:3], name
            assert h["bucket_limit"] == lim and h["bucket"] == cnt, name
            assert abs(h["sum"] - stats[3]) <= C.SUM_BOUND * math.fsum(np.abs(value.astype(np.float64).reshape(-1))), name
            assert abs(h["sum_squares"] - stats[4]) <= C.SUM_BOUND * stats[4], name
