#!/usr/bin/env python
"""Prices the one-launch batch norms of the FC tail per layer width: bn_act_small_fwd / _bwd on [1024 x c] with mask,
moving averages and dparam as the step calls them, 4 rotating buffer sets, REPS launches captured into one graph and
replayed (so the figure is the device's time per dependent launch, not the host's), median of ROUNDS replays.

The library under test is whatever HYPEL_LIB_PATH names (default: the tree's).  Building elementwise.hip with
-DHYPEL_SMALL_FORCE_TX=4 | 8 | 16 | 32 pins the stripe width of every launch, which is how the widths behind
small_stripe() were priced against each other (profiles/fc_tail_stamps.txt):

  python tools/exp/fc_tail_probe.py [--rows 1024] [--widths 15,45,...] [--tag NAME]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hypelcnn_amd.backend import HipBackend, Ref  # noqa: E402

REPS, ROUNDS, SETS = 40, 15, 4
EPS, DECAY, ALPHA, ACT_LRELU = 1e-3, 0.95, 0.18, 1


def price(hip, rows, c):
    rng = np.random.default_rng(c)
    up = lambda a: hip.upload(a.astype(np.float32))  # noqa: E731
    sets = []
    for _ in range(SETS):
        sets.append({"y": up(rng.standard_normal((rows, c))), "dz": up(rng.standard_normal((rows, c))),
                     "mask": up((rng.random((rows, c)) < 0.7) / 0.7), "z": hip.empty(rows * c), "dy": hip.empty(rows * c)})
    beta, mean, rstd = up(rng.standard_normal(c)), hip.empty(c), hip.empty(c)
    mm, mv, dp = up(np.zeros(c)), up(np.ones(c)), up(np.zeros(c))
    fwd, bwd = [], []
    for i in range(REPS):
        s = sets[i % SETS]
        fwd.append(hip.bind("bn_act_small_fwd", (Ref(s["y"]), c, rows, c, EPS, Ref(beta), ACT_LRELU, ALPHA, Ref(s["mask"]), c,
                                                 Ref(mean), Ref(rstd), Ref(mm), Ref(mv), DECAY, Ref(s["z"]), c)))
        bwd.append(hip.bind("bn_act_small_bwd", (Ref(s["dz"]), c, Ref(s["y"]), c, rows, c, Ref(mean), Ref(rstd), Ref(beta),
                                                 ACT_LRELU, ALPHA, Ref(s["mask"]), c, Ref(s["dy"]), c, Ref(dp), 1)))
    out = []
    for launches in (fwd, bwd):
        launches[0]()
        hip.synchronize()
        replay = hip.capture(launches)
        replay()
        hip.synchronize()
        times = []
        for _ in range(ROUNDS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(hip.stream)
            replay()
            b.record(hip.stream)
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / REPS)
        out.append((float(np.median(times)), float(np.min(times))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--widths", default="15,45,108,135,326,405,980,7105")
    ap.add_argument("--tag", default=os.path.basename(os.environ.get("HYPEL_LIB_PATH", "tree")))
    a = ap.parse_args()
    hip = HipBackend()
    print(f"# {a.tag}: rows {a.rows}; us per launch, median (min) of {ROUNDS} replays of {REPS} launches")
    print(f"# {'c':>6} {'fwd':>16} {'bwd':>16}")
    tf = tb = 0.0
    for c in [int(w) for w in a.widths.split(",")]:
        (f, fm), (b, bm) = price(hip, a.rows, c)
        tf, tb = tf + f, tb + b
        print(f"  {c:6d} {f:8.2f} ({fm:5.2f}) {b:8.2f} ({bm:5.2f})")
    print(f"  {'sum':>6} {tf:8.2f}         {tb:8.2f}")


if __name__ == "__main__":
    main()
