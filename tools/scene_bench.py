#!/usr/bin/env python3
"""Times the scene-preparation launches (csrc/scene.hip) on synthetic rasters of the contest scenes' sizes, beside
their byte floors -- one read of the source raster plus, for the prepare launch, one write of the float32 scene -- and
the host BasicDataSet on the same arrays.  Needs a HIP device.

    python tools/scene_bench.py [--reps 5] [--neighborhood 4] [--skip-host]
prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hypelcnn_amd.backend import OUT_DTYPES, SCENE_RANK_WS_WORDS, HipBackend, Ref  # noqa: E402
from hypelcnn_amd.common.common_nn_ops import BasicDataSet  # noqa: E402
from hypelcnn_amd.common.device_scene import DeviceBasicDataSet, _Source  # noqa: E402

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


def case(be, name, casi, nb, reps, clip, skip_host):
    src = _Source(be, casi)
    item, bands = src.dtype.itemsize, src.bands
    n_src = src.h * src.w * bands
    n_out = (src.h + 2 * nb) * (src.w + 2 * nb) * bands
    out2 = be.zeros(2 * bands * item, torch.uint8)
    ws_e = be.empty(2 * 1024 * bands * item, torch.uint8)
    ws_r = be.empty(bands * SCENE_RANK_WS_WORDS * 4, torch.uint8)
    scene = be.empty(n_out, torch.float32)
    lo = be.zeros(bands * item, torch.uint8)
    scale = be.upload(np.full(bands, 1234.5, np.float32))
    smap = be.upload((np.random.default_rng(0).random((src.h + 2 * nb) * (src.w + 2 * nb)) < 0.3).astype(np.uint8))
    sums = be.zeros((2 * bands + 2) * 8, torch.uint8)
    ws_s = be.empty(2048 * 2 * (bands + 1) * 8, torch.uint8)
    g = src.geometry()
    launches = {
        "extrema": (lambda: be.call("scene_extrema", src.ref, src.code, *g, None, None, Ref(out2),
                                    Ref(out2, bands * item), Ref(ws_e), 1024), n_src * item),
        "prepare": (lambda: be.call("scene_prepare_f32", src.ref, src.code, *g, nb, None, Ref(lo), Ref(scale),
                                    Ref(scene)), n_src * item + n_out * 4),
        "masked_sums": (lambda: be.call("scene_masked_sums", Ref(scene), Ref(smap), src.h + 2 * nb, src.w + 2 * nb,
                                        bands, Ref(sums), Ref(sums, 2 * bands * 8), Ref(ws_s), 2048), n_out * 4),
    }
    if clip:
        n = src.h * src.w
        launches["rank_select"] = (lambda: be.call("scene_rank_select_u16", src.ref, *g, int(0.95 * (n - 1)),
                                                   int(0.95 * (n - 1)) + 1, Ref(out2), Ref(out2, bands * 2), Ref(ws_r)),
                                   2 * n_src * item)  # the two radix levels each read the raster once
    rec = {"case": name, "shape": [src.h, src.w, bands], "strides": list(src.strides), "dtype": str(src.dtype)}
    for key, (fn, nbytes) in launches.items():
        ms = timed(be, fn, reps)
        rec[key] = {"ms": round(ms, 4), "floor_ms": round(nbytes / HBM_GBS / 1e6, 4),
                    "GBps": round(nbytes / ms / 1e6, 1)}
    t0 = time.perf_counter()
    DeviceBasicDataSet(None, casi, None, nb, True, casi_min=0 if clip else None, backend=be,
                       clip_percentile=95 if clip else None)
    be.synchronize()
    rec["device_data_set_ms"] = round((time.perf_counter() - t0) * 1e3, 2)  # upload and scalar downloads included
    if not skip_host:
        t0 = time.perf_counter()
        host = np.array(casi, copy=True, order="K")
        if clip:
            np.clip(host, None, np.percentile(host, 95, axis=[0, 1]).astype(host.dtype), out=host)
        BasicDataSet(None, host, None, nb, True, casi_min=0 if clip else None)
        rec["host_data_set_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--neighborhood", type=int, default=4)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args(argv)
    be = HipBackend()
    rng = np.random.default_rng(0)
    grss = rng.integers(0, 20000, (349, 1905, 144), dtype=np.uint16)
    case(be, "grss2013 349x1905x144 uint16 chunky", grss, a.neighborhood, a.reps, False, a.skip_host)
    del grss
    stored = rng.integers(0, 4096, (360, 320, 400 + 110), dtype=np.uint16)  # [band, column, row + blank margin]
    avon = np.swapaxes(stored[:, :, 55:-55], 0, 2)
    case(be, "avon 400x320x360 uint16 [band, column, row] window", avon, a.neighborhood, a.reps, True, a.skip_host)


if __name__ == "__main__":
    main()
