#!/usr/bin/env python3
"""Times the three band-PCA launches (csrc/pca.hip) on synthetic padded scenes of the contest scenes' sizes, beside their
byte floors -- one read of the scene's interior per fit pass; for the projection one read of the padded scene plus one
write of k / C of it -- at the float4 copy rate DESIGN quotes, and scikit-learn's PCA on the host for scale (skipped
where scikit-learn is not installed).  Needs a HIP device.

    python tools/pca_bench.py [--reps 5] [--neighborhood 2] [--components 16] [--skip-host]
prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hypelcnn_amd.backend import HipBackend, Ref  # noqa: E402
from hypelcnn_amd.classic.decomposition import BandPCA, band_sums_ws_doubles, scatter_ws_doubles  # noqa: E402

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


def case(be, name, h, w, bands, nb, k, reps, skip_host):
    rng = np.random.default_rng(0)
    hp, wp = h + 2 * nb, w + 2 * nb
    # raw uint16-like values: a smooth spectrum per pixel + noise
    base = rng.uniform(2000.0, 12000.0, bands).astype(np.float32)
    scene = torch.from_numpy(base[None, :] + rng.standard_normal((hp * wp, bands), dtype=np.float32) * 30.0)
    scene = scene.reshape(hp, wp, bands).to(be.device)
    flat = scene.reshape(-1)
    origin, sy, sx, n = nb * (wp + 1) * bands, wp * bands, bands, h * w
    sums, scatter = be.zeros(bands, torch.float64), be.zeros(bands * bands, torch.float64)
    ws_sums = be.empty(band_sums_ws_doubles(n, bands), torch.float64)
    ws_scatter = be.empty(scatter_ws_doubles(n, bands), torch.float64)
    be.call("pca_band_sums_f64", Ref(flat, origin), h, w, bands, sy, sx, Ref(sums), Ref(ws_sums), ws_sums.numel())
    mean = be.upload((sums.cpu().numpy() / n).astype(np.float32))
    weights = be.upload((rng.standard_normal((bands, k)) / np.sqrt(bands)).astype(np.float32))
    out = be.empty(hp * wp * k)
    launches = {
        "band_sums": (lambda: be.call("pca_band_sums_f64", Ref(flat, origin), h, w, bands, sy, sx, Ref(sums), Ref(ws_sums),
                                      ws_sums.numel()), n * bands * 4),
        "scatter": (lambda: be.call("pca_scatter_f64", Ref(flat, origin), h, w, bands, sy, sx, Ref(mean), Ref(scatter),
                                    Ref(ws_scatter), ws_scatter.numel()), n * bands * 4),
        "project": (lambda: be.call("pca_project_f32", Ref(flat), 1, hp * wp, bands, hp * wp * bands, bands, 0, Ref(mean),
                                    Ref(weights), k, Ref(out), k), hp * wp * (bands + k) * 4),
    }
    rec = {"case": name, "shape": [h, w, bands], "neighborhood": nb, "components": k}
    for key, (fn, nbytes) in launches.items():
        ms = timed(be, fn, reps)
        rec[key] = {"ms": round(ms, 4), "floor_ms": round(nbytes / HBM_GBS / 1e6, 4), "GBps": round(nbytes / ms / 1e6, 1)}
    rec["scatter"]["TFLOPs"] = round(2.0 * n * bands * bands / rec["scatter"]["ms"] / 1e9, 2)  # of the full c x c product
    t0 = time.perf_counter()
    pca = BandPCA(k, backend=be).fit(scene[nb:hp - nb, nb:wp - nb, :])
    be.synchronize()
    rec["fit_ms"] = round((time.perf_counter() - t0) * 1e3, 2)  # both passes, the downloads and the host eigh
    if not skip_host:
        try:
            from sklearn.decomposition import PCA
        except ImportError:
            PCA = None
        if PCA is not None:
            # in float64: on the float32 array NumPy's column means are off by tens of units at this size, and
            # scikit-learn's variances with them (NOTES.md, "Band PCA")
            host = scene[nb:hp - nb, nb:wp - nb, :].reshape(n, bands).cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            theirs = PCA(k, svd_solver="full").fit(host)
            rec["sklearn_fit_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            t0 = time.perf_counter()
            theirs.transform(host)
            rec["sklearn_transform_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            rec["explained_variance_rel_diff"] = float(np.max(np.abs(pca.explained_variance_ - theirs.explained_variance_)
                                                              / theirs.explained_variance_))
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--neighborhood", type=int, default=2)
    ap.add_argument("--components", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args(argv)
    be = HipBackend()
    case(be, "grss2013 349x1905x144", 349, 1905, 144, a.neighborhood, a.components, a.reps, a.skip_host)
    case(be, "avon 400x320x360", 400, 320, 360, a.neighborhood, a.components, a.reps, a.skip_host)


if __name__ == "__main__":
    main()
