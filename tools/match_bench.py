#!/usr/bin/env python3
"""Times the launches of utilities/lidar_matcher.py (csrc/match.hip) at the contest geometry beside their floors: band 8
of the GRSS2013 scene (349 x 1905) enlarged 5 times against a GRSS2018 band without its last 350 rows and 75 columns,
enlarged 2 times.  The size of the GRSS2018 HSI raster is not recorded in the loader's documentation; 1202 x 4172 (the
contest's 1 m grid) is assumed here -- pass --template_shape to use another.  The numerator's floor is its
2 * hout * wout * HT * WT FLOP at the measured 155 TF of the fp32 matrix pipe; the other launches are quoted against the
bytes they have to move once at the measured copy rate.  For scale, where SciPy is importable, scipy.signal.fftconvolve
of the same enlarged rasters on the host (the numerator alone).  Needs a HIP device.

    python tools/match_bench.py [--reps 3] [--skip-host] [--contiguous] [--splits N] [--image_shape 349,1905] [--template_shape 1202,4172]
prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hypelcnn_amd.backend import HipBackend, Ref  # noqa: E402
from hypelcnn_amd.common import device_match as dm  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of the MI355X
MATRIX_F32_TFLOPS = 155.0  # measured rate of v_mfma_f32_32x32x2_f32
IMAGE_BANDS, IMAGE_BAND, IMAGE_SCALE = 144, 8, 5
TEMPLATE_BANDS, TEMPLATE_BAND, TEMPLATE_SCALE, CROP = 48, 2, 2, (350, 75)


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


def shape(text):
    h, w = (int(v) for v in text.split(","))
    return h, w


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--contiguous", action="store_true", help="copy each band out of its scene first (sx = 1)")
    ap.add_argument("--splits", type=int, default=None, help="blocks per output tile (default: device_match's choice)")
    ap.add_argument("--image_shape", type=shape, default=(349, 1905))
    ap.add_argument("--template_shape", type=shape, default=(1202, 4172))
    a = ap.parse_args(argv)
    be = HipBackend()
    gen = torch.Generator(device=be.device).manual_seed(0)
    # pixel-major scenes in HBM, as the loaders leave them; the bands are read in place
    image_scene = torch.rand((*a.image_shape, IMAGE_BANDS), generator=gen, device=be.device)
    template_scene = torch.rand((*a.template_shape, TEMPLATE_BANDS), generator=gen, device=be.device)
    image_band = image_scene[:, :, IMAGE_BAND]
    template_band = template_scene[:a.template_shape[0] - CROP[0], :a.template_shape[1] - CROP[1], TEMPLATE_BAND]
    if a.contiguous:
        image_band, template_band = image_band.contiguous(), template_band.contiguous()
    img = dm._Band(be, image_band, IMAGE_SCALE, "image")
    tpl = dm._Band(be, template_band, TEMPLATE_SCALE, "template")
    hout, wout = img.H - tpl.H + 1, img.W - tpl.W + 1
    n = hout * wout
    splits = a.splits or dm.choose_splits(hout, wout, tpl.H, tpl.W)
    num, ws = be.empty(n), be.empty(splits * n)
    energy, e_t = be.empty(n, torch.float64), be.empty(1, torch.float64)
    ws_rows, ws_tpl = be.empty(img.h * wout, torch.float64), be.empty(tpl.h, torch.float64)
    scores, record = be.empty(n), be.empty(2, torch.int64)
    figure, top = be.empty(img.H * img.W, torch.uint8), be.upload(np.ones(1, np.float32))
    flop = 2.0 * n * tpl.H * tpl.W
    launches = {
        # the FLOP of the definition; the bytes (both bands once, the surface once) are negligible beside them
        "ccorr": (lambda: be.call("match_ccorr_f32", img.ref, *img.geometry(), tpl.ref, *tpl.geometry(), Ref(num),
                                  Ref(ws), splits), flop / MATRIX_F32_TFLOPS / 1e9),
        # the band once, the row sums written and read once, the surface written
        "image_energy": (lambda: be.call("match_window_energy_f64", img.ref, *img.geometry(), tpl.H, tpl.W, Ref(energy),
                                         Ref(ws_rows)), (4 * img.h * img.w + 16 * img.h * wout + 8 * n) / HBM_GBS / 1e6),
        "template_energy": (lambda: be.call("match_window_energy_f64", tpl.ref, *tpl.geometry(), tpl.H, tpl.W, Ref(e_t),
                                            Ref(ws_tpl)), (4 * tpl.h * tpl.w + 16 * tpl.h + 8) / HBM_GBS / 1e6),
        "best": (lambda: be.call("match_best_f32", Ref(num), Ref(energy), Ref(e_t), hout, wout, Ref(scores), Ref(record)),
                 (4 * n + 8 * n + 4 * n + 16) / HBM_GBS / 1e6),
        "render": (lambda: be.call("match_render_u8", img.ref, *img.geometry(), Ref(top), Ref(figure)),
                   (4 * img.h * img.w + img.H * img.W) / HBM_GBS / 1e6),
    }
    rec = {"image": [img.h, img.w, IMAGE_SCALE], "template": [tpl.h, tpl.w, TEMPLATE_SCALE],
           "template_raster_assumed": list(a.template_shape), "bands_read": "copied out" if a.contiguous else "in place",
           "surface": [hout, wout], "splits": splits,
           "gflop": round(flop / 1e9, 1)}
    for key, (fn, floor_ms) in launches.items():
        ms = timed(be, fn, a.reps)
        rec[key] = {"ms": round(ms, 4), "floor_ms": round(floor_ms, 5)}
    rec["ccorr"]["tflops"] = round(flop / rec["ccorr"]["ms"] / 1e9, 1)
    rec["ccorr"]["of_floor"] = round(rec["ccorr"]["floor_ms"] / rec["ccorr"]["ms"], 3)
    t0 = time.perf_counter()
    found = dm.match_template(be, img, tpl, splits=splits)
    rec["match_template_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    rec["top_left"], rec["score"] = list(found.top_left), found.score
    if not a.skip_host:
        try:
            from scipy.signal import fftconvolve
        except ImportError:
            fftconvolve = None
        if fftconvolve is not None:
            big = np.repeat(np.repeat(image_scene[:, :, IMAGE_BAND].cpu().numpy(), IMAGE_SCALE, 0), IMAGE_SCALE, 1)
            small = np.repeat(np.repeat(tpl_host(template_scene, a.template_shape), TEMPLATE_SCALE, 0), TEMPLATE_SCALE, 1)
            t0 = time.perf_counter()
            host = fftconvolve(big, small[::-1, ::-1], mode="valid")
            rec["host"] = {"what": "scipy.signal.fftconvolve (numerator only)",
                           "ms": round((time.perf_counter() - t0) * 1e3, 1),
                           "max_rel_diff": float(np.abs(host - num.cpu().numpy().reshape(hout, wout)).max()
                                                 / np.abs(host).max())}
    print(json.dumps(rec), flush=True)


def tpl_host(template_scene, full):
    return template_scene[:full[0] - CROP[0], :full[1] - CROP[1], TEMPLATE_BAND].cpu().numpy()


if __name__ == "__main__":
    main()
