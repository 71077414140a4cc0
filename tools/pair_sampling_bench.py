#!/usr/bin/env python3
"""Times the pixel-pairing launches (csrc/pairs.hip) on a synthetic scene of the GRSS2013 raster's size, beside their
byte floors -- the bytes each launch has to read and write once -- then the device path of the three samplers end to
end, and the host samplers' wall time on the host copy of the same scene.  Needs a HIP device.

    python tools/pair_sampling_bench.py [--reps 5] [--h 349 --w 1905 --bands 144] [--skip-host]
prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hypelcnn_amd.backend import COMPACT_TILE, HipBackend, Ref  # noqa: E402
from hypelcnn_amd.common.common_nn_ops import BasicDataSet  # noqa: E402
from hypelcnn_amd.common.device_scene import DeviceBasicDataSet  # noqa: E402
from hypelcnn_amd.gan import gan_sampling_methods as S  # noqa: E402
from hypelcnn_amd.gan.wrapper_registry import get_sampling_map  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of the MI355X, the ceiling the floors are quoted against


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


def blobs(h, w, rng):
    """uint8 [h, w] shadow map: one disc of radius 6 to 24 per 16 000 pixels, a few per cent of the scene"""
    count = max(1, h * w // 16000)
    yy, xx = np.mgrid[0:h, 0:w]
    smap = np.zeros((h, w), np.uint8)
    for cy, cx, r in zip(rng.random(count) * h, rng.random(count) * w, 6 + rng.random(count) * 18):
        smap[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 1
    return smap


class Loader:
    def __init__(self, targets, classes):
        self._targets, self._classes = targets, classes

    def read_targets(self, target_image_path):
        return self._targets

    def get_class_count(self):
        return range(0, self._classes)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--h", type=int, default=349)
    ap.add_argument("--w", type=int, default=1905)
    ap.add_argument("--bands", type=int, default=144)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args(argv)
    be = HipBackend()
    rng = np.random.default_rng(0)
    h, w, n = a.h, a.w, a.h * a.w
    smap = blobs(h, w, rng)
    map_d = be.upload(smap)
    out8, ws32 = be.empty(n, torch.uint8), be.empty(n, torch.int32)
    reach, margin = S.device_dilate(be, map_d, h, w, 20), S.device_dilate(be, map_d, h, w, 2)
    shadow_m, lit_m = S.device_pair_masks(be, map_d, n, reach, margin)
    n_lit = int(lit_m.sum())
    points, count = be.empty(2 * n, torch.int32), be.empty(1, torch.int32)
    ws_c = be.empty((n + COMPACT_TILE - 1) // COMPACT_TILE, torch.int32)
    expanded = be.empty(2 * n, torch.int32)
    n_sh = int(shadow_m.sum())
    sh_points = S.device_compact(be, shadow_m, h, w)
    launches = {
        # row pass: the map in, the int32 distances out; column pass: the distances in (once at best), the mask out
        "dilate_r20": (lambda: be.call("mask_dilate_l1_u8", Ref(map_d), h, w, 20, Ref(out8), Ref(ws32)), 10 * n),
        "dilate_r2": (lambda: be.call("mask_dilate_l1_u8", Ref(map_d), h, w, 2, Ref(out8), Ref(ws32)), 10 * n),
        "pair_masks": (lambda: be.call("pair_masks_u8", Ref(map_d), Ref(reach), Ref(margin), n, Ref(shadow_m), Ref(lit_m)),
                       5 * n),
        # the mask twice (count, scatter) and the selected points out
        "compact_lit": (lambda: be.call("mask_compact_points_i32", Ref(lit_m), h, w, Ref(points), n, Ref(count), Ref(ws_c)),
                        2 * n + 8 * n_lit),
        "expand": (lambda: be.call("points_expand_i32", Ref(sh_points.reshape(-1)), n_sh, n // n_sh, 0, Ref(expanded)),
                   8 * n_sh + 8 * n_sh * (n // n_sh)),
    }
    rec = {"case": "launches", "shape": [h, w], "shadowed": n_sh, "ring": n_lit}
    for key, (fn, nbytes) in launches.items():
        ms = timed(be, fn, a.reps)
        rec[key] = {"ms": round(ms, 4), "floor_ms": round(nbytes / HBM_GBS / 1e6, 6), "GBps": round(nbytes / ms / 1e6, 1)}
    print(json.dumps(rec), flush=True)

    casi = rng.integers(0, 20000, (h, w, a.bands), dtype=np.uint16)
    data_set = DeviceBasicDataSet(None, casi, None, 0, True, backend=be)
    ys, xs = np.nonzero(rng.random((h, w)) < 0.02)
    loader = Loader(np.stack([xs, ys, rng.integers(0, 15, xs.size)], axis=1).astype(int), 15)
    host_set = None
    if not a.skip_host:
        host_set = BasicDataSet(None, casi, None, 0, True)
    for method, sampler in get_sampling_map().items():
        if method == "dummy":
            continue
        be.synchronize()
        t0 = time.perf_counter()
        normal, shadow = sampler.get_sample_pairs_device(data_set, loader, smap, be, hsi_only=True)
        be.synchronize()
        rec = {"case": method, "pairs": int(normal.shape[0]), "bands": a.bands,
               "device_ms": round((time.perf_counter() - t0) * 1e3, 2),
               "pair_bytes": 2 * int(normal.numel()) * 4}
        del normal, shadow
        if host_set is not None:
            t0 = time.perf_counter()
            sampler.get_sample_pairs(host_set, loader, smap)
            rec["host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        assert data_set.downloaded() == []
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
