"""Kernel SVC (hypelcnn_amd.classic.svc) on a SyntheticDataLoader scene: fit and whole-scene prediction, one JSON line
with the wall times, every launch's event time next to its byte / FLOP floor (bytes / 6.2 TB/s, the streaming rate
DESIGN.md uses; products: 2 m n k FLOP / 157 TFLOP/s, the fp32 matrix rate the split-operand path is measured against),
the SMO iterations per pair and, where scikit-learn is importable, the same fit and prediction on the CPU for scale.

    python tools/svm_bench.py [--path grss2013] [--kernel rbf] [--gamma 1e-9] [--c 1e4] [--tol 1e-3] [--sklearn 1]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hypelcnn_amd.backend import HipBackend  # noqa: E402
from hypelcnn_amd.classic.svc import SVC  # noqa: E402
from hypelcnn_amd.common.common_nn_ops import SceneArrays, get_loader_from_name  # noqa: E402
from hypelcnn_amd.importer.InMemoryImporter import InMemoryImporter  # noqa: E402

STREAM_BYTES_PER_S, FP32_MATRIX_FLOPS = 6.2e12, 157e12


def floor_us(name, a):
    """Algorithmic floor of one launch from its arguments (include/hypel.h order)."""
    if name == "seg_gemm_f32":
        return None  # filled in by the caller, who knows m and k
    if name == "svm_center_norms_f32":
        return 2 * 4 * a[2] * a[3] / STREAM_BYTES_PER_S * 1e6
    if name == "svm_kernel_apply_f32":
        return 2 * 4 * a[2] * a[3] / STREAM_BYTES_PER_S * 1e6
    if name == "svm_vote":
        return 4 * a[2] * (a[3] * (a[3] - 1) // 2) / STREAM_BYTES_PER_S * 1e6
    return None


class TimedBackend:
    """HipBackend whose launches are event-timed one by one (synchronising: for the per-launch table only)."""

    def __init__(self, inner):
        self.inner, self.log = inner, []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def call(self, name, *args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream())
        self.inner.call(name, *args)
        b.record(torch.cuda.current_stream())
        b.synchronize()
        self.log.append((name, args, a.elapsed_time(b) * 1e3))


def table(log):
    rows = {}
    for name, args, us in log:
        fl = floor_us(name, args)
        r = rows.setdefault(name, {"launches": 0, "us": 0.0, "floor_us": 0.0 if fl is not None else None})
        r["launches"] += 1
        r["us"] += us
        if fl is not None:
            r["floor_us"] += fl
    return {k: {kk: (round(vv, 1) if isinstance(vv, float) else vv) for kk, vv in v.items()} for k, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", default="grss2013")
    ap.add_argument("--kernel", default="rbf")
    ap.add_argument("--gamma", default="1e-9")
    ap.add_argument("--c", type=float, default=1e4)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--neighborhood", type=int, default=2)
    ap.add_argument("--sklearn", type=int, default=1)
    args = ap.parse_args()
    gamma = "scale" if args.gamma == "scale" else float(args.gamma)
    kw = dict(kernel=args.kernel, gamma=gamma, C=args.c, degree=1 if args.kernel == "poly" else 3, tol=args.tol)
    tr, _, va, _, _, shape, _ = InMemoryImporter().read_data_set("SyntheticDataLoader", args.path, 0.1, 0,
                                                                 args.neighborhood, False)
    X, y = tr.data.reshape(len(tr.data), -1), tr.labels
    loader = get_loader_from_name("SyntheticDataLoader", args.path)
    data_set = loader.load_data(args.neighborhood, False)
    h, w = shape[:2]
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    targets = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(xs.size, dtype=int)], axis=1)
    hip = HipBackend()
    result = {"tool": "svm_bench", "config": {"path": args.path, **kw}, "train_rows": int(len(X)),
              "features": int(X.shape[1]), "scene_pixels": int(h * w)}

    def run(backend):
        arrays = SceneArrays()
        arrays.feed(data_set, targets, backend)
        raster = torch.zeros(h * w, dtype=torch.uint8, device=hip.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model = SVC(backend=backend, **kw).fit(X, y)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        model.predict_scene(arrays, raster, w)
        torch.cuda.synchronize()
        return model, t1 - t0, time.perf_counter() - t1, raster.cpu().numpy()

    run(hip)  # warm-up: code objects, allocator
    model, fit_s, scene_s, labels = run(hip)
    result.update(fit_s=round(fit_s, 4), scene_predict_s=round(scene_s, 4), n_sv=int(len(model.support_)),
                  smo_iterations={"max": int(model.n_iter_.max()), "sum": int(model.n_iter_.sum()),
                                  "pairs": int(len(model.n_iter_))})
    timed = TimedBackend(hip)
    run(timed)
    result["launches"] = table(timed.log)
    l, f, n_sv = len(X), X.shape[1], len(model.support_)
    result["product_floor_us"] = {"fit_K": round(2.0 * l * l * f / FP32_MATRIX_FLOPS * 1e6, 1),
                                  "scene_K": round(2.0 * h * w * n_sv * f / FP32_MATRIX_FLOPS * 1e6, 1)}
    if args.sklearn:
        try:
            from sklearn.svm import SVC as SK
        except ImportError:
            SK = None
        if SK is not None:
            t0 = time.perf_counter()
            sk = SK(cache_size=1000, **kw).fit(X, y)
            t1 = time.perf_counter()
            scene = np.stack([data_set.get_data_point(int(px), int(py)).reshape(-1) for px, py, _ in targets])
            t2 = time.perf_counter()
            ref = sk.predict(scene)
            result["sklearn_cpu"] = {"fit_s": round(t1 - t0, 3), "scene_predict_s": round(time.perf_counter() - t2, 3),
                                     "label_agreement": float((ref == labels).mean())}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
