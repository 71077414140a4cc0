#!/usr/bin/env python3
"""Times the two band-ratio launches (csrc/band_ratio.hip) at the validation hooks' size, 6 000 x 144, and at a scene's
pairs, 500 000 x 144 and 500 000 x 360, beside their byte floors at the device-to-device copy rate measured in the same
run -- the ratio: two reads and one write of the matrix; the rank select: one read -- and beside what they replace, the
reference's three numpy.percentile calls on the host.  The select reads the matrix once for level 1 and once per pair
of ranks for each of the three levels below, so `select_reads` = 1 + 3 * ceil(ranks / 2) (6 ranks for the 10th, 50th
and 90th percentile: 10 reads);
`select_GBps` is that traffic over the time.  Inputs are 16-bit quantised spectra, so ties are as common as in a scene;
`select_spread_ms` and `select_ties90_ms` time the same select on values without ties and with 90 % of every column at
one value.
Needs a HIP device.

    python tools/band_ratio_bench.py [--reps 20] [--skip-host]
prints one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hypelcnn_amd.backend import COLUMN_RANK_WS_WORDS, HipBackend, Ref  # noqa: E402
from hypelcnn_amd.common.band_ratio import band_ratio_stats  # noqa: E402
from hypelcnn_amd.common.device_scene import percentile_ranks  # noqa: E402

SHAPES = ((6000, 144), (500000, 144), (500000, 360))


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


def spectra(n, bands, seed):
    rng = np.random.default_rng(seed)
    lit = rng.integers(2000, 60000, (n, bands)).astype(np.float32) / np.float32(65535)
    shadow = np.round(lit * 65535 * (0.4 + 0.1 * rng.standard_normal((n, bands)))).astype(np.float32) / np.float32(65535)
    lit[rng.random(n) < 0.01, 0] = 0.0  # a few rows the mask drops
    return shadow, lit


def case(be, n, bands, reps, rate, skip_host):
    shadow, lit = spectra(n, bands, n + bands)
    num, den = be.upload(shadow), be.upload(lit)
    ratio, ok, count = be.empty(n * bands), be.empty(n, torch.uint8), be.empty(1, torch.int64)
    scale = be.upload(np.linspace(1.5, 2.5, bands).astype(np.float32))
    ratio_call = be.bind("band_ratio_f32", (Ref(num), bands, Ref(den), bands, n, bands, Ref(scale), Ref(ratio), bands,
                                            Ref(ok), Ref(count)))
    ratio_ms = timed(be, ratio_call, reps)
    kept = int(count.cpu()[0])
    ranks = sorted({r for q in (10, 50, 90) for r in percentile_ranks(kept, q)[:2]})
    out = be.empty(len(ranks) * bands)
    ws = be.empty(bands * COLUMN_RANK_WS_WORDS, torch.int32)
    host_ranks = torch.tensor(ranks, dtype=torch.int64)
    select_call = be.bind("column_rank_select_f32", (Ref(ratio), bands, n, bands, Ref(ok), kept, Ref(host_ranks),
                                                     len(ranks), Ref(out), Ref(ws)))
    select_ms = timed(be, select_call, reps)
    # what ties cost the LDS atomics: the same select, all rows kept, on values without ties and with 90 % of every
    # column at one value (a wavefront-wide merge of equal counters could win back no more than the difference)
    full_ranks = torch.tensor(sorted({r for q in (10, 50, 90) for r in percentile_ranks(n, q)[:2]}), dtype=torch.int64)
    spread = torch.rand(n * bands, device=ratio.device) * 4 - 1
    tied = torch.where(torch.rand(n * bands, device=ratio.device) < 0.9, torch.full_like(spread, 1.25), spread)
    by_data = {}
    for name, x in (("spread", spread), ("ties90", tied)):
        call = be.bind("column_rank_select_f32", (Ref(x), bands, n, bands, None, n, Ref(full_ranks), int(full_ranks.numel()),
                                                  Ref(out), Ref(ws)))
        by_data[name] = timed(be, call, reps)
    del spread, tied
    band_ratio_stats(be, num.view(n, bands), den.view(n, bands), scale)  # (the first call loads torch's kernels)
    be.synchronize()
    t0 = time.perf_counter()
    stats = band_ratio_stats(be, num.view(n, bands), den.view(n, bands), scale)
    be.synchronize()
    whole_ms = (time.perf_counter() - t0) * 1e3
    matrix = n * bands * 4
    reads = 1 + 3 * ((len(ranks) + 1) // 2)
    rec = {"rows": n, "bands": bands, "kept": kept, "ranks": len(ranks), "copy_GBps": round(rate, 1),
           "ratio_ms": round(ratio_ms, 4), "ratio_floor_ms": round(3 * matrix / rate / 1e6, 4),
           "select_ms": round(select_ms, 4), "select_floor_ms": round(matrix / rate / 1e6, 4), "select_reads": reads,
           "select_GBps": round(reads * matrix / select_ms / 1e6, 1), "stats_with_host_ms": round(whole_ms, 3),
           "select_spread_ms": round(by_data["spread"], 4), "select_ties90_ms": round(by_data["ties90"], 4)}
    if not skip_host:
        host = ratio.cpu().numpy().reshape(n, bands)
        t0 = time.perf_counter()
        host = host[np.isfinite(host).all(axis=1)]
        want = [np.percentile(host, q, axis=0) for q in (50, 10, 90)]
        rec["host_numpy_percentile_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["max_abs_difference_p50"] = float(np.abs(stats["p50"] - want[0]).max())
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args(argv)
    be = HipBackend()
    rate = copy_rate_gbs(be, 5)
    for n, bands in SHAPES:
        case(be, n, bands, a.reps, rate, a.skip_host)


if __name__ == "__main__":
    main()
