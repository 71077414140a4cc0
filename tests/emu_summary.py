"""TEST INFRASTRUCTURE: numpy twin of hypel_tensor_summary_f32 (include/hypel.h), attached to
tests/emu_backend.EmuBackend on import.  Written from the header: the bucket of a finite element is
numpy.searchsorted(limits, float64(v), side="right") -- upper_bound on the table itself -- and the sums are math.fsum,
the correctly rounded sums of the exact float64 values and squares."""
import math
import sys

import numpy as np

from hypelcnn_amd.backend import SUMMARY_MAX_LIMITS, SUMMARY_SLICE
from tests.emu_backend import EmuBackend
from tests.emu_scene import _typed

DBL_MAX = sys.float_info.max


def summarize(values, limits):
    """-> (min, max, num, sum, sum_squares), non-finite count, int64 bucket counts of one float32 tensor"""
    v = np.asarray(values, np.float32).reshape(-1)
    fin = np.isfinite(v)
    d = v[fin].astype(np.float64)
    b = np.minimum(np.searchsorted(limits, d, side="right"), len(limits) - 1)
    counts = np.bincount(b, minlength=len(limits)).astype(np.int64)
    stats = (float(d.min()) if d.size else DBL_MAX, float(d.max()) if d.size else -DBL_MAX, float(d.size),
             math.fsum(d), math.fsum(d * d))  # a float32 squared is exact in float64
    return stats, int(v.size - d.size), counts


def _k_tensor_summary_f32(self, base, table, n_segs, limits, n_limits, stats, nonfinite, buckets, ws, ws_slices):
    assert n_segs > 0 and 1 <= n_limits <= SUMMARY_MAX_LIMITS and ws_slices >= 0
    tab = _typed(table, np.int64, 2 * n_segs).reshape(n_segs, 2)
    lim = _typed(limits, np.float64, n_limits)
    assert (np.diff(lim) >= 0).all()
    assert ws.t.numel() - ws.off >= n_segs + 1 + 6 * ws_slices
    bad = _typed(nonfinite, np.int64, n_segs)
    if sum((int(s) + SUMMARY_SLICE - 1) // SUMMARY_SLICE for s in tab[:, 1] if s > 0) != ws_slices:
        bad[:] = -1
        return
    x = _typed(base, np.float32)
    out = _typed(stats, np.float64, 5 * n_segs).reshape(n_segs, 5)
    cnt = _typed(buckets, np.int64, n_segs * n_limits).reshape(n_segs, n_limits)
    for s, (off, size) in enumerate(tab):
        assert off >= 0 and off + max(size, 0) <= x.size
        out[s], bad[s], cnt[s] = summarize(x[off:off + max(size, 0)], lim)


EmuBackend.k_tensor_summary_f32 = _k_tensor_summary_f32
