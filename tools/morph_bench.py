#!/usr/bin/env python3
"""Times the four grey-scale morphology launches (csrc/morph.hip) and a whole extended morphological profile on synthetic
padded scenes of the contest scenes' sizes -- 8 principal components, GRSS2013 with its LiDAR channel, radii 2,4,6,8 --
beside their byte floors at the float4 copy rate DESIGN quotes: keys, store and erode / dilate one read and one write of
the image, a sweep three image streams (marker in, mask, marker out).  scipy.ndimage.grey_erosion and a NumPy
reconstruction by one-pixel steps on the host, one channel each, for scale (skipped where scipy is not installed).
Needs a HIP device.

    python tools/morph_bench.py [--reps 10] [--neighborhood 2] [--components 8] [--radii 2,4,6,8] [--skip-host]
prints one JSON line per case."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hypelcnn_amd.backend import MORPH_DILATE, MORPH_DISK, MORPH_ERODE, HipBackend, Ref  # noqa: E402
from hypelcnn_amd.classic.morphology import MorphologicalProfile  # noqa: E402

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


def blobs(rng, hp, wp, c, cell=12):
    """float32 [hp, wp, c]: flat regions of about `cell` pixels with a little noise on top, as principal components of a
    scene of fields and roofs look -- white noise would make every reconstruction walk long geodesic paths"""
    coarse = rng.standard_normal((-(-hp // cell), -(-wp // cell), c)).astype(np.float32)
    fine = np.repeat(np.repeat(coarse, cell, axis=0), cell, axis=1)[:hp, :wp]
    return fine + 0.05 * rng.standard_normal((hp, wp, c)).astype(np.float32)


def host_reconstruct(marker, mask):
    """reconstruction by dilation of one channel by one-pixel steps -> (the limit, steps)"""
    m = np.minimum(marker, mask)
    for steps in range(m.size):
        padded = np.pad(m, 1, mode="constant", constant_values=-np.inf)
        nxt = m.copy()
        for dy in range(3):
            for dx in range(3):
                np.maximum(nxt, padded[dy:dy + m.shape[0], dx:dx + m.shape[1]], out=nxt)
        np.minimum(nxt, mask, out=nxt)
        if np.array_equal(nxt, m):
            return m, steps
        m = nxt
    return m, m.size


def case(be, name, h, w, c, lidar, nb, radii, reps, skip_host):
    rng = np.random.default_rng(0)
    hp, wp = h + 2 * nb, w + 2 * nb
    casi = torch.from_numpy(blobs(rng, hp, wp, c)).to(be.device)
    lidar_d = torch.from_numpy(blobs(rng, hp, wp, lidar)).to(be.device) if lidar else None
    flat = casi.reshape(-1)
    origin, sy, sx, n = nb * (wp + 1) * c, wp * c, c, h * w
    keys, eroded, other = (be.empty(n * c, torch.int32) for _ in range(3))
    changed = be.zeros(1, torch.int32)
    out = be.empty(hp * wp * c)
    image_bytes = n * c * 4
    rec = {"case": name, "shape": [h, w, c], "lidar": lidar, "neighborhood": nb, "radii": list(radii)}

    def note(key, fn, nbytes):
        ms = timed(be, fn, reps)
        rec[key] = {"ms": round(ms, 4), "floor_ms": round(nbytes / HBM_GBS / 1e6, 4), "GBps": round(nbytes / ms / 1e6, 1)}

    note("keys", lambda: be.call("morph_keys_u32", Ref(flat, origin), h, w, c, sy, sx, Ref(keys)), 2 * image_bytes)
    for r in radii:
        for op_name, op in (("erode", MORPH_ERODE), ("dilate", MORPH_DILATE)):
            note(f"{op_name}_r{r}", lambda: be.call("morph_erode_dilate_u32", Ref(keys), h, w, c, r, MORPH_DISK, op,
                                                    Ref(eroded)), 2 * image_bytes)
    be.call("morph_erode_dilate_u32", Ref(keys), h, w, c, radii[len(radii) // 2], MORPH_DISK, MORPH_ERODE, Ref(eroded))
    note("sweep_first", lambda: be.call("morph_reconstruct_sweep_u32", Ref(eroded), Ref(keys), h, w, c, MORPH_DILATE,
                                        Ref(other), Ref(changed)), 3 * image_bytes)
    limit, sweeps = MorphologicalProfile(radii, backend=be)._reconstruct(eroded.clone(), keys, h, w, c, MORPH_DILATE, "bench")
    rec["sweeps_to_the_limit"] = sweeps
    note("sweep_at_the_limit", lambda: be.call("morph_reconstruct_sweep_u32", Ref(limit), Ref(keys), h, w, c, MORPH_DILATE,
                                               Ref(other), Ref(changed)), 3 * image_bytes)
    note("store", lambda: be.call("morph_profile_store_f32", Ref(keys), h, w, c, nb, Ref(out), c, 0, 1),
         image_bytes + hp * wp * c * 4)
    scene = types.SimpleNamespace(casi_dev=casi, lidar_dev=lidar_d, neighborhood=nb, casi_scale=1,
                                  get_scene_shape=lambda: [h, w])
    for by_reconstruction in (True, False):
        profile = MorphologicalProfile(radii, by_reconstruction=by_reconstruction, backend=be)
        profile.transform_scene(scene)  # warm
        be.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            profile.transform_scene(scene)
        be.synchronize()
        key = "profile" if by_reconstruction else "profile_plain"
        rec[key + "_ms"] = round((time.perf_counter() - t0) * 1e3 / reps, 2)  # wall: launches and the `changed` reads
        if by_reconstruction:
            rec["profile_sweeps"] = sum(profile.sweeps_.values())
    if not skip_host:
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            r = radii[len(radii) // 2]
            yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
            host = casi[nb:hp - nb, nb:wp - nb, 0].cpu().numpy()
            t0 = time.perf_counter()
            low = ndimage.grey_erosion(host, footprint=yy * yy + xx * xx <= r * r, mode="constant", cval=np.inf)
            rec[f"scipy_grey_erosion_r{r}_one_channel_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            t0 = time.perf_counter()
            _, steps = host_reconstruct(low, host)
            rec["numpy_reconstruction_one_channel_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            rec["numpy_reconstruction_steps"] = steps
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--neighborhood", type=int, default=2)
    ap.add_argument("--components", type=int, default=8)
    ap.add_argument("--radii", type=str, default="2,4,6,8")
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args(argv)
    radii = tuple(int(v) for v in a.radii.split(","))
    be = HipBackend()
    case(be, "grss2013 349x1905, 8 components + lidar", 349, 1905, a.components, 1, a.neighborhood, radii, a.reps, a.skip_host)
    case(be, "avon 400x320, 8 components", 400, 320, a.components, 0, a.neighborhood, radii, a.reps, a.skip_host)


if __name__ == "__main__":
    main()
