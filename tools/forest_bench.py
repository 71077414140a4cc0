"""Random forest (hypelcnn_amd.classic.forest) on a SyntheticDataLoader scene: fit, per-launch event times, and
whole-scene serving on a synthetic scene of the real GRSS2013 size (349 x 1905 pixels, 144 + 1 bands) through both
paths -- hypel_forest_predict_scene straight on the padded scene, next to its byte floor (the scene read once, the
raster written once, at 6.2 TB/s, the streaming rate DESIGN.md uses), and the chunked hypel_gather_patches_f32 +
hypel_forest_predict_rows it replaces (floor: every patch written once and read once) -- one JSON line.  Where
scikit-learn is importable, RandomForestClassifier(n_jobs=16) on the CPU for scale: its fit, and its prediction of
--sklearn_rows scene rows.

--estimator extra_trees measures hypelcnn_amd.classic.forest.ExtraTreesForest the same way (scikit-learn's
ExtraTreesClassifier for scale) and adds `fit_levels`: per level the event times of hypel_forest_split_random and
hypel_forest_split_apply_thr beside the records, the rows they cover and the byte floor of the search -- per record its
rows of one xt column twice (the range, then the counts) plus order, y and weight once, 20 bytes a row, at 6.2 TB/s.

--diagnostics R replaces the scene part by the forest diagnostics on the same problem: the per-launch event times of
hypel_forest_oob_rows, hypel_forest_importances_f64 and hypel_forest_permuted_hits (one group per band, R repeats), the
wall times of the three methods, and scikit-learn's oob_score=True and sklearn.inspection.permutation_importance at
n_jobs=16 for orientation.

    python tools/forest_bench.py [--estimator forest] [--path grss2013] [--trees 50] [--max_features 24]
                                 [--scene_h 349] [--scene_w 1905] [--diagnostics 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hypelcnn_amd.backend import HipBackend  # noqa: E402
from hypelcnn_amd.classic.forest import ExtraTreesForest, ForestClassifier  # noqa: E402
from hypelcnn_amd.common.common_nn_ops import SceneArrays, get_loader_from_name  # noqa: E402
from hypelcnn_amd.importer.InMemoryImporter import InMemoryImporter  # noqa: E402

STREAM_BYTES_PER_S = 6.2e12


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
        self.log.append((name, a.elapsed_time(b) * 1e3))


def table(log):
    rows = {}
    for name, us in log:
        r = rows.setdefault(name, {"launches": 0, "us": 0.0, "max_us": 0.0})
        r["launches"] += 1
        r["us"] += us
        r["max_us"] = max(r["max_us"], us)
    return {k: {kk: (round(vv, 1) if isinstance(vv, float) else vv) for kk, vv in v.items()} for k, v in rows.items()}


def level_table(log, level_rows, max_features):
    """extra_trees: one row per level from the launch log (one search and one apply launch a level, in order)"""
    search = [us for name, us in log if name == "forest_split_random"]
    apply = [us for name, us in log if name == "forest_split_apply_thr"]
    out = []
    for level, (nodes, rows) in enumerate(level_rows):
        floor_us = 20.0 * rows * max_features / STREAM_BYTES_PER_S * 1e6
        out.append({"level": level, "nodes": nodes, "records": nodes * max_features, "node_rows": rows,
                    "split_random_us": round(search[level], 1), "split_random_floor_us": round(floor_us, 2),
                    "split_apply_thr_us": round(apply[level], 1)})
    return out


def timed(fn, repeats=3):
    """best wall time of `repeats` synchronised calls, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def diagnostics(args, model, log, hip, train, validation, channels, result):
    """--diagnostics R: per-launch event times of hypel_forest_oob_rows (training rows), hypel_forest_importances_f64 and
    hypel_forest_permuted_hits (validation rows, one group per band, R repeats); for orientation only, scikit-learn's
    extra cost of oob_score=True at fit and sklearn.inspection.permutation_importance (per COLUMN, its own stream) at
    n_jobs=16."""
    (X, y), (Xv, yv) = train, validation
    del log.log[:]
    model._be = log
    oob = model.out_of_bag(X, y)
    model.feature_importances()
    model.permutation_importance(Xv, yv, n_repeats=args.diagnostics, group_mod=channels, seed=0)
    model._be = hip
    wall = {"out_of_bag_s": timed(lambda: model.out_of_bag(X, y)), "feature_importances_s": timed(model.feature_importances),
            "permutation_importance_s": timed(lambda: model.permutation_importance(
                Xv, yv, n_repeats=args.diagnostics, group_mod=channels, seed=0), repeats=1)}
    result["diagnostics"] = {"launches": table(log.log), "wall": {k: round(v, 5) for k, v in wall.items()},
                             "oob_score": oob, "oob_rows_without_vote": int((model.oob_votes_ == 0).sum()),
                             "n_used": model.importances_n_used_, "train_rows": int(len(X)),
                             "validation_rows": int(len(Xv)), "groups": int(channels), "repeats": args.diagnostics}
    if not args.sklearn:
        return
    try:
        from sklearn.ensemble import ExtraTreesClassifier, RandomForestClassifier
        from sklearn.inspection import permutation_importance
    except ImportError:
        return
    cls = ExtraTreesClassifier if args.estimator == "extra_trees" else RandomForestClassifier
    fits = {}
    for oob_score in (False, True):
        t0 = time.perf_counter()
        sk = cls(args.trees, max_features=min(args.max_features, X.shape[1]), n_jobs=16, bootstrap=True,
                 oob_score=oob_score, random_state=0).fit(X, y)
        fits[oob_score] = time.perf_counter() - t0
    t0 = time.perf_counter()
    sk.feature_importances_
    t1 = time.perf_counter()
    sk.set_params(n_jobs=1)  # (the columns are the parallel axis below)
    permutation_importance(sk, Xv, yv, n_repeats=args.diagnostics, n_jobs=16, random_state=0)
    t2 = time.perf_counter()
    result["diagnostics"]["sklearn_cpu"] = {"fit_s": round(fits[False], 3), "fit_oob_score_s": round(fits[True], 3),
                                            "oob_score": float(sk.oob_score_), "feature_importances_s": round(t1 - t0, 4),
                                            "permutation_importance_s": round(t2 - t1, 2),
                                            "permutation_columns": int(X.shape[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--diagnostics", type=int, default=0,
                    help="R > 0: instead of the scene, the forest diagnostics (out-of-bag, importances, R permutation "
                         "repeats per band) launch by launch; extra_trees is then grown with bootstrap")
    ap.add_argument("--estimator", default="forest", choices=("forest", "extra_trees"))
    ap.add_argument("--path", default="grss2013")
    ap.add_argument("--trees", type=int, default=50)
    ap.add_argument("--max_features", type=int, default=24)
    ap.add_argument("--neighborhood", type=int, default=2)
    ap.add_argument("--scene_h", type=int, default=349)
    ap.add_argument("--scene_w", type=int, default=1905)
    ap.add_argument("--fit_repeats", type=int, default=2,
                    help="timed fits after one warm-up; 0: fit_s is the wall time of the one event-timed fit "
                         "(its per-launch synchronisation included), for tree counts whose host draws take minutes")
    ap.add_argument("--sklearn", type=int, default=1)
    ap.add_argument("--sklearn_rows", type=int, default=20000)
    args = ap.parse_args()
    tr, _, va, _, _, _, _ = InMemoryImporter().read_data_set("SyntheticDataLoader", args.path, 0.1, 0, args.neighborhood,
                                                             False)
    X, y = tr.data.reshape(len(tr.data), -1), tr.labels
    Xv, yv = va.data.reshape(len(va.data), -1), va.labels
    hip = HipBackend()
    kw = dict(n_estimators=args.trees, max_features=args.max_features)
    if args.diagnostics:
        kw["bootstrap"] = True
    result = {"tool": "forest_bench", "config": {"estimator": args.estimator, "path": args.path, **kw},
              "train_rows": int(len(X)), "features": int(X.shape[1])}
    extra = args.estimator == "extra_trees"
    level_rows = []

    class Estimator(ExtraTreesForest if extra else ForestClassifier):
        def _level_done(self, level, active, n_active, *tables):
            if self.count_levels:
                level_rows.append((n_active, int(active[:4 * n_active].view(n_active, 4)[:, 2].sum())))
    Estimator.count_levels = False

    if args.fit_repeats:
        fit_s = timed(lambda: Estimator(backend=hip, **kw).fit(X, y), repeats=args.fit_repeats)
    log = TimedBackend(hip)
    Estimator.count_levels = True
    t0 = time.perf_counter()
    model = Estimator(backend=log, **kw).fit(X, y)
    if not args.fit_repeats:
        fit_s = time.perf_counter() - t0
    Estimator.count_levels = False
    model._be = hip
    result.update(fit_s=round(fit_s, 4), nodes=int(len(model.feature_)), levels=int(model.n_levels_),
                  validation_oa=float((model.predict(Xv) == yv).mean()))
    result["fit_launches"] = table(log.log)
    if extra:
        result["fit_levels"] = level_table(log.log, level_rows, model._resolve_max_features(X.shape[1]))
    result["fit_launch_sum_s"] = round(sum(us for _, us in log.log) * 1e-6, 4)
    if args.diagnostics:
        diagnostics(args, model, log, hip, (X, y), (Xv, yv), tr.data.shape[3], result)
        print(json.dumps(result))
        return

    # whole-scene serving on a scene of the real size (the model's features are the same window of the same bands)
    big = f"{args.path}:h={args.scene_h}:w={args.scene_w}"
    data_set = get_loader_from_name("SyntheticDataLoader", big).load_data(args.neighborhood, False)
    h, w = data_set.get_scene_shape()[:2]
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    targets = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(xs.size, dtype=int)], axis=1)
    arrays = SceneArrays()
    arrays.feed(data_set, targets, hip)
    raster = torch.zeros(h * w, dtype=torch.uint8, device=hip.device)
    scene_bytes = 4 * (arrays.casi.numel() + (0 if arrays.lidar is None else arrays.lidar.numel())) + h * w
    patch_bytes = 2 * 4 * h * w * X.shape[1] + h * w
    direct_s = timed(lambda: model.predict_scene(arrays, raster, w, direct=True))
    direct = raster.cpu().numpy().copy()
    gather_s = timed(lambda: model.predict_scene(arrays, raster, w, direct=False), repeats=1)
    same = bool(np.array_equal(direct, raster.cpu().numpy()))
    result["scene"] = {"pixels": int(h * w), "direct_s": round(direct_s, 5), "gather_rows_s": round(gather_s, 5),
                       "direct_floor_s": round(scene_bytes / STREAM_BYTES_PER_S, 6),
                       "gather_rows_floor_s": round(patch_bytes / STREAM_BYTES_PER_S, 6),
                       "direct_over_floor": round(direct_s / (scene_bytes / STREAM_BYTES_PER_S), 1),
                       "gather_over_direct": round(gather_s / direct_s, 2), "same_raster": same}
    if args.sklearn:
        try:
            from sklearn.ensemble import ExtraTreesClassifier, RandomForestClassifier
            if extra:
                RandomForestClassifier = ExtraTreesClassifier
        except ImportError:
            RandomForestClassifier = None
        if RandomForestClassifier is not None:
            t0 = time.perf_counter()
            sk = RandomForestClassifier(args.trees, max_features=min(args.max_features, X.shape[1]), n_jobs=16,
                                        random_state=0).fit(X, y)
            t1 = time.perf_counter()
            pick = np.random.default_rng(0).choice(h * w, min(args.sklearn_rows, h * w), replace=False)
            rows = np.stack([data_set.get_data_point(int(px), int(py)).reshape(-1) for px, py, _ in targets[pick]])
            t2 = time.perf_counter()
            ref = sk.predict(rows)
            t3 = time.perf_counter()
            result["sklearn_cpu"] = {"fit_s": round(t1 - t0, 3), "predict_rows": int(len(rows)),
                                     "predict_s": round(t3 - t2, 3),
                                     "scene_predict_s_scaled": round((t3 - t2) * h * w / len(rows), 1),
                                     "validation_oa": float((sk.predict(Xv) == yv).mean()),
                                     "label_agreement": float((ref == direct[pick]).mean())}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
