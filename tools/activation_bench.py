#!/usr/bin/env python3
"""Times the activation range and histogram launches (csrc/activation.hip: hypel_view_range_f32,
hypel_view_histogram_f32) on views the size of GRSS2013 HYPELCNN's first tap at batch 1024 -- 1024 * 81 * 480 floats, 480
uniform bins between the data's extremes --

    contiguous   cols == ld, normal(0, 1) values
    strided      the same number of elements as cols = ld / 2 columns of twice the rows, at an odd element offset
    all_equal    contiguous, one value everywhere (a controlled input: every wavefront agrees on its bin)

beside the floor of reading every element once -- 4 bytes per element at the copy rate measured in the same run -- and
beside hypel_tensor_summary_f32 on the contiguous data with the interior edges plus DBL_MAX as its limits table (the same
bins; it also sums in fp64 and estimates from a logarithm).  Needs a HIP device.

    python tools/activation_bench.py [--reps 200] [--rounds 5] [--batch 1024]
prints one JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hypelcnn_amd.backend import HipBackend, Ref  # noqa: E402
from hypelcnn_amd.common.device_summary import TensorSummary  # noqa: E402

PIXELS, WIDTH, BINS = 81, 480, 480


def timed(be, fn, reps):
    fn()
    be.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def copy_rate_gbs(be, reps):
    """read + write bytes per second of a device-to-device copy of 1 GiB"""
    src, dst = be.empty(1 << 28), be.empty(1 << 28)
    src.normal_()
    ms = timed(be, lambda: dst.copy_(src), reps)
    return 2 * src.numel() * 4 / ms / 1e6


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    a = ap.parse_args(argv)
    be = HipBackend()
    rate = copy_rate_gbs(be, a.reps)
    rows = a.batch * PIXELS
    elements = rows * WIDTH
    data = be.empty(2 * elements + 8)
    data.normal_()
    lo, hi = float(data.min()), float(data.max())
    edges = np.linspace(lo, hi, BINS + 1)
    edges_dev = be.upload(edges)
    out_range = be.upload(np.asarray([3.4e38, -3.4e38], np.float32))
    count, counts, outside = be.zeros(2, torch.int64), be.zeros(BINS, torch.int64), be.zeros(1, torch.int64)

    def report(case, range_ms, hist_ms, extra=None):
        floor = elements * 4 / rate / 1e6
        rec = {"case": case, "elements": elements, "bins": BINS, "range_ms": round(range_ms, 4),
               "histogram_ms": round(hist_ms, 4), "floor_ms": round(floor, 4),
               "range_over_floor": round(range_ms / floor, 2), "histogram_over_floor": round(hist_ms / floor, 2),
               "copy_GBps": round(rate, 1)}
        rec.update(extra or {})
        print(json.dumps(rec), flush=True)
        return rec

    def view(off, n_rows, ld, cols):
        r = timed(be, lambda: be.call("view_range_f32", Ref(data, off), n_rows, ld, cols, Ref(out_range), Ref(count)),
                  a.reps)
        h = timed(be, lambda: be.call("view_histogram_f32", Ref(data, off), n_rows, ld, cols, Ref(edges_dev), BINS,
                                      Ref(counts), Ref(outside)), a.reps)
        return r, h

    # the yardstick: the tensor-summary launch over the same contiguous elements and the same bins
    limits = np.concatenate([edges[1:-1], [sys.float_info.max]])
    ts = TensorSummary(be, data, [(0, elements)], be.upload(limits), limits.size)
    rounds = []  # the two alternate, so that a drift of the clocks meets both
    for _ in range(a.rounds):
        summary_ms = timed(be, ts.launch, a.reps)
        rounds.append((summary_ms,) + view(0, rows, WIDTH, WIDTH))
    summary_ms, r, h = (float(np.median([x[k] for x in rounds])) for k in range(3))
    report("contiguous", r, h, {"tensor_summary_ms": round(summary_ms, 4),
                                "histogram_over_tensor_summary": round(h / summary_ms, 3),
                                "rounds": [[round(v, 4) for v in x] for x in rounds]})
    r, h = view(1, 2 * rows, WIDTH, WIDTH // 2)
    report("strided", r, h, {"ld": WIDTH, "cols": WIDTH // 2, "offset": 1})
    data.fill_(0.0371)
    uniform = report("all_equal", *view(0, rows, WIDTH, WIDTH))
    return uniform


if __name__ == "__main__":
    main()
