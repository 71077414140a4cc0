#!/usr/bin/env python3
"""Times the tensor-summary launch (csrc/summary.hip, hypel_tensor_summary_f32) over the real variable tables of
HYPELCNN and DUALCNN and over one synthetic 256 M-element segment of trained-weight-like values (normal, sigma 0.05),
beside the floor of reading every element once -- 4 bytes per element at the float4 copy rate measured in the same run --
and, for the models, beside the host path it replaces (`variable_norms`: sess.get_variable of every variable and
numpy.linalg.norm).  Needs a HIP device.

    python tools/summary_bench.py [--reps 5] [--synthetic-elements 268435456] [--skip-models]
prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from hypelcnn_amd.backend import HipBackend  # noqa: E402
from hypelcnn_amd.common.device_summary import TensorSummary, VariableSummarizer  # noqa: E402
from hypelcnn_amd.common.tb_events import default_bucket_limits  # noqa: E402


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


def report(name, elements, segments, ms, rate, extra=None):
    rec = {"case": name, "elements": int(elements), "segments": int(segments), "summary_ms": round(ms, 4),
           "floor_ms": round(elements * 4 / rate / 1e6, 4), "GBps": round(elements * 4 / ms / 1e6, 1),
           "copy_GBps": round(rate, 1)}
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)


def model_case(be, workload, reps, rate):
    ctx, _, _, _ = bench.build_model(8, be, workload)
    sess = ctx.session()
    summarizer = VariableSummarizer(sess)
    ms = timed(be, summarizer.launch, reps)
    t0 = time.perf_counter()
    results = summarizer.run()
    with_copy_ms = (time.perf_counter() - t0) * 1e3  # launch + the per-variable results to the host
    t0 = time.perf_counter()
    norms = {n: float(np.linalg.norm(sess.get_variable(n))) for n in sess.variable_names()}
    host_ms = (time.perf_counter() - t0) * 1e3
    worst = max(abs(np.sqrt(results[n]["sum_squares"]) - norms[n]) / (norms[n] + 1e-30) for n in norms)
    elements = sum(int(results[n]["num"]) + results[n]["nonfinite"] for n in results)
    report(workload, elements, len(results), ms, rate,
           {"summary_with_results_ms": round(with_copy_ms, 3), "host_variable_norms_ms": round(host_ms, 1),
            "max_rel_norm_difference": float(worst)})


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--synthetic-elements", type=int, default=1 << 28)
    ap.add_argument("--skip-models", action="store_true")
    a = ap.parse_args(argv)
    be = HipBackend()
    rate = copy_rate_gbs(be, a.reps)
    limits = default_bucket_limits()
    base = be.empty(a.synthetic_elements)
    base.normal_(0.0, 0.05)
    ts = TensorSummary(be, base, [(0, a.synthetic_elements)], be.upload(limits), limits.size)
    report("synthetic normal(0, 0.05)", a.synthetic_elements, 1, timed(be, ts.launch, a.reps), rate)
    del ts, base
    if not a.skip_models:
        for workload in ("hypelcnn", "dualcnn"):
            model_case(be, workload, a.reps, rate)


if __name__ == "__main__":
    main()
