"""TEST INFRASTRUCTURE: inputs of the tensor-summary tests and the comparison against the twin (tests/emu_summary.py),
shared by the host tests (EmuBackend) and the GPU tests (HipBackend)."""
import math

import numpy as np
import torch

from hypelcnn_amd.backend import SUMMARY_SLICE, Ref
from hypelcnn_amd.common.device_summary import TensorSummary
from hypelcnn_amd.common.tb_events import default_bucket_limits
from tests.emu_summary import summarize

LIMITS = default_bucket_limits()
FLT_MAX, FLT_MIN = np.finfo(np.float32).max, np.finfo(np.float32).tiny
SUB_MIN, SUB_MAX = np.float32(1e-45), np.nextafter(np.float32(FLT_MIN), np.float32(0))
SENTINEL = np.float32(12345.0)
SUM_BOUND = 64 * 2.0 ** -53  # |sum - fsum| <= 64 * 2^-53 * sum|x|: any pairwise / tree fp64 sum of < 2^64 exact terms


def boundary_values():
    """the two float32 neighbours of each of the 1548 finite non-zero limits, +-0, the extreme subnormals, +-FLT_MIN,
    +-FLT_MAX"""
    lim = LIMITS[(LIMITS != 0.0) & (np.abs(LIMITS) < 1e300)]
    assert lim.size == 1548
    with np.errstate(over="ignore"):
        near = lim.astype(np.float32)
    assert not (near.astype(np.float64) == lim).any()  # no limit but 0.0 is a float32
    below = np.where(near.astype(np.float64) < lim, near, np.nextafter(near, np.float32(-np.inf)))
    above = np.nextafter(below, np.float32(np.inf))
    assert (below.astype(np.float64) < lim).all() and (above.astype(np.float64) > lim).all()
    extra = np.asarray([0.0, -0.0, SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX],
                       np.float32)
    return np.concatenate([below, above, extra]).astype(np.float32)


def layout(tensors, odd_offsets=True, order=None, seed=0):
    """Packs float32 tensors into one buffer filled with SENTINEL: gaps between the segments, odd element offsets (no
    16-byte alignment), table rows in `order`.  -> buffer, [(offset, size)] in table order, the tensors in table order"""
    order = list(range(len(tensors))) if order is None else list(order)
    rng = np.random.default_rng(seed)
    offs, pos = [], 1
    for t in tensors:
        pos += int(rng.integers(1, 9))
        if odd_offsets and pos % 2 == 0:
            pos += 1
        offs.append(pos)
        pos += t.size
    buf = np.full(pos + 8, SENTINEL, np.float32)
    for o, t in zip(offs, tensors):
        buf[o:o + t.size] = t
    return buf, [(offs[i], tensors[i].size) for i in order], [tensors[i] for i in order]


def launch(be, buf, segments, limits=LIMITS):
    """-> stats [n, 5], nonfinite [n], buckets [n, n_limits] as numpy, straight from the launch"""
    ts = TensorSummary(be, be.upload(buf), segments, be.upload(np.asarray(limits, np.float64)), len(limits))
    ts.launch()
    be.synchronize()
    return ts.results()


def check_against_twin(got, tensors, limits=LIMITS):
    stats, nonfinite, buckets = got
    for i, t in enumerate(tensors):
        want, want_bad, want_counts = summarize(t, limits)
        where = f"segment {i} (size {t.size})"
        assert nonfinite[i] == want_bad, where
        diff = np.flatnonzero(buckets[i] != want_counts)
        assert diff.size == 0, (where, diff[:8], buckets[i][diff[:8]], want_counts[diff[:8]])
        assert stats[i, 0] == want[0] and stats[i, 1] == want[1] and stats[i, 2] == want[2], (where, stats[i], want)
        fin = t[np.isfinite(t)].astype(np.float64)
        abs_sum, sq_sum = math.fsum(np.abs(fin)), want[4]
        print(f"{where}: |sum - fsum| = {abs(stats[i, 3] - want[3]):.3e} (bound {SUM_BOUND * abs_sum:.3e}), "
              f"|sum_squares - fsum| = {abs(stats[i, 4] - want[4]):.3e} (bound {SUM_BOUND * sq_sum:.3e})")
        assert abs(stats[i, 3] - want[3]) <= SUM_BOUND * abs_sum, where
        assert abs(stats[i, 4] - want[4]) <= SUM_BOUND * sq_sum, where


def shape_case():
    """sizes 0, 1, 63, 64, 65, 4097 and 3 * 2^20 + 5 (split over blocks) at odd offsets with sentinel gaps, the table out
    of address order"""
    rng = np.random.default_rng(7)
    sizes = [0, 1, 63, 64, 65, 4097, 3 * 2 ** 20 + 5, SUMMARY_SLICE, SUMMARY_SLICE + 1]
    tensors = [(rng.standard_normal(n) * 0.05).astype(np.float32) for n in sizes]
    return layout(tensors, order=[6, 2, 0, 8, 4, 1, 7, 5, 3], seed=3)
