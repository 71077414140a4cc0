#!/usr/bin/env python3
"""Times the launches of utilities/reveal_shadow_targets.py (csrc/components.hip) beside their byte floors -- the bytes
each has to read and write once -- on three masks: discs on a raster of MUUFL Gulfport's size (325 x 220), discs on one
of GRSS2013's (349 x 1905), and random pixels on 2404 x 8344 at a density next to the percolation threshold of the
8-connected square lattice (1 - 0.5927), where components are largest and most tangled.  For scale, the same labelling
on the host: scipy.ndimage.label where scipy is importable, a plain-Python flood fill otherwise.  Needs a HIP device.

    python tools/shadow_targets_bench.py [--reps 5] [--bands 64] [--skip-host] [--skip-large]
prints one JSON line per mask."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hypelcnn_amd.backend import COMPACT_TILE, HipBackend, Ref  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of the MI355X, the ceiling the floors are quoted against
N_CLASSES = 11
PERCOLATION = 1 - 0.5927


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


def discs(h, w, rng):
    """uint8 [h, w]: one disc of radius 3 to 12 per 4 000 pixels, a few per cent of the scene"""
    count = max(1, h * w // 4000)
    yy, xx = np.mgrid[0:h, 0:w]
    smap = np.zeros((h, w), np.uint8)
    for cy, cx, r in zip(rng.random(count) * h, rng.random(count) * w, 3 + rng.random(count) * 9):
        smap[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 1
    return smap


def flood_fill_count(mask):
    h, w = mask.shape
    pw = w + 2
    padded = np.zeros((h + 2, pw), np.uint8)
    padded[1:-1, 1:-1] = mask != 0
    todo = bytearray(padded.tobytes())
    steps = (-pw - 1, -pw, -pw + 1, -1, 1, pw - 1, pw, pw + 1)
    count = 0
    for start in range(len(todo)):
        if todo[start]:
            count += 1
            todo[start] = 0
            stack = [start]
            while stack:
                p = stack.pop()
                for s in steps:
                    if todo[p + s]:
                        todo[p + s] = 0
                        stack.append(p + s)
    return count


def host_label(mask):
    """-> (what ran, components, milliseconds)"""
    t0 = time.perf_counter()
    try:
        from scipy import ndimage
    except ImportError:
        return "python flood fill", flood_fill_count(mask), (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    count = ndimage.label(mask != 0, structure=np.ones((3, 3)))[1]
    return "scipy.ndimage.label", int(count), (time.perf_counter() - t0) * 1e3


def bench(be, name, mask, bands, reps, skip_host):
    h, w = mask.shape
    n = h * w
    rng = np.random.default_rng(n)
    targets = rng.integers(0, N_CLASSES, (h, w)).astype(np.uint8)
    targets[mask != 0] = 6
    map_d, targets_d = be.upload(mask), be.upload(targets)
    root, ws, status = be.empty(n, torch.int32), be.empty(n, torch.int32), be.zeros(1, torch.int32)
    comp, count = be.empty(n, torch.int32), be.zeros(1, torch.int32)
    ws_c = be.empty((n + COMPACT_TILE - 1) // COMPACT_TILE, torch.int32)
    be.call("components_label_u8", Ref(map_d), h, w, Ref(root), Ref(ws), Ref(status))
    be.call("components_compact_i32", Ref(root), h, w, Ref(comp), Ref(count), Ref(ws_c))
    k = int(count.cpu()[0])
    assert int(status.cpu()[0]) == 0
    votes, size, winner = (be.empty(max(k, 1) * N_CLASSES, torch.int32), be.empty(max(k, 1), torch.int32),
                           be.empty(max(k, 1), torch.uint8))
    out = be.empty(n, torch.uint8)
    scene = be.upload(rng.random((n, bands), dtype=np.float32))
    r_minus_1 = be.upload(rng.random(bands, dtype=np.float32) * 3)
    corrected = be.empty(n * bands, torch.float32)
    launches = {
        # the mask in, the roots out (the parent table in between is written once and read at least once on top)
        "label": (lambda: be.call("components_label_u8", Ref(map_d), h, w, Ref(root), Ref(ws), Ref(status)), 5 * n),
        "compact": (lambda: be.call("components_compact_i32", Ref(root), h, w, Ref(comp), Ref(count), Ref(ws_c)), 8 * n),
        "votes": (lambda: be.call("components_votes_i32", Ref(targets_d), Ref(comp), h, w, k, N_CLASSES, 0xC0, Ref(votes),
                                  Ref(size), Ref(winner)), 5 * n + 4 * k * (N_CLASSES + 1) + k),
        "relabel": (lambda: be.call("components_relabel_u8", Ref(targets_d), Ref(comp), Ref(winner), h, w, 1, Ref(out)),
                    6 * n + k),
        "correct": (lambda: be.call("shadow_correct_f32", Ref(scene), 0, h, w, bands, w * bands, bands, 1, Ref(map_d),
                                    Ref(r_minus_1), Ref(corrected)), 8 * n * bands + n),
    }
    rec = {"case": name, "shape": [h, w], "inside": int((mask != 0).sum()), "components": k, "bands": bands}
    for key, (fn, nbytes) in launches.items():
        ms = timed(be, fn, reps)
        rec[key] = {"ms": round(ms, 4), "floor_ms": round(nbytes / HBM_GBS / 1e6, 6), "GBps": round(nbytes / ms / 1e6, 1)}
    rec["largest"] = int(size.max()) if k else 0
    if not skip_host:
        what, host_count, ms = host_label(mask)
        assert host_count == k, (host_count, k)
        rec["host"] = {"what": what, "ms": round(ms, 2)}
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bands", type=int, default=64)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args(argv)
    be = HipBackend()
    rng = np.random.default_rng(0)
    bench(be, "gulfport_325x220", discs(325, 220, rng), a.bands, a.reps, a.skip_host)
    bench(be, "grss2013_349x1905", discs(349, 1905, rng), a.bands, a.reps, a.skip_host)
    if not a.skip_large:
        mask = (rng.random((2404, 8344)) < PERCOLATION).astype(np.uint8)
        bench(be, "percolation_2404x8344", mask, 4, a.reps, a.skip_host)  # 4 bands: the scene stays under 1 GiB


if __name__ == "__main__":
    main()
