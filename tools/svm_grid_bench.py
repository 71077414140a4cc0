"""SVC grid search (hypelcnn_amd.classic.model_selection.GridSearchSVC) on the fixture cases of tests/svm_grid_cases.py:
one JSON line per case with
  grid_s             wall time of the batched search, per job order ("c_desc", "plain"), after a warm-up run
  loop_s             the yardstick: the same grid as a loop of per-cell SVC(...).fit + .predict on the same splits, i.e.
                     what the search costs with the single-fit entry points alone; ratio = loop_s / grid_s
  launches           event time per entry point of one (synchronising) timed run
  jobs / iterations  job count and the iteration histogram (min / median / max / sum) of the smo_grid launches
  tail_share_modelled  NOT a measurement: share of the smo_grid time left after half of the workgroups have retired, estimated from the
                     per-job iteration counts: jobs are replayed in issue order on slots = CUs x resident workgroups,
                     a job's length taken as its iteration count (a model of the schedule, not a trace)
  sklearn_cpu_s      GridSearchCV on the host for scale, only if scikit-learn imports.

    python tools/svm_grid_bench.py [--cases small,grss2013] [--loop 1] [--sklearn 0]"""
import argparse
import heapq
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hypelcnn_amd.backend import HipBackend  # noqa: E402
from hypelcnn_amd.classic.model_selection import JOB_ORDERS, GridSearchSVC, StratifiedShuffleSplit  # noqa: E402
from hypelcnn_amd.classic.svc import SVC  # noqa: E402
from tests import svm_grid_cases as G  # noqa: E402
from tools.svm_bench import TimedBackend  # noqa: E402

SLOTS = 256 * 2  # the model's parallel slots: 256 CUs x 2 resident workgroups (a workgroup holds up to 48 KB of LDS)


def cv():
    return StratifiedShuffleSplit(n_splits=G.N_SPLITS, test_size=G.TEST_SIZE, random_state=G.SEED)


def tail_share(lengths, slots=SLOTS):
    """Replay jobs of the given lengths, in order, on `slots` parallel slots: (makespan - time at which half of the jobs
    have retired) / makespan."""
    free = [0.0] * min(slots, len(lengths))
    heapq.heapify(free)
    ends = []
    for ln in lengths:
        t = heapq.heappop(free) + float(ln)
        ends.append(t)
        heapq.heappush(free, t)
    ends.sort()
    return (ends[-1] - ends[len(ends) // 2]) / ends[-1] if ends[-1] > 0 else 0.0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="small,grss2013")
    ap.add_argument("--loop", type=int, default=1)
    ap.add_argument("--sklearn", type=int, default=0)
    args = ap.parse_args()
    hip = HipBackend()
    for case in args.cases.split(","):
        X, y = G.load_case_data(case)
        grid = G.grid_of(case)
        result = {"tool": "svm_grid_bench", "case": case, "path": G.CASES[case]["path"], "rows": int(len(y)),
                  "features": int(X.shape[1]), "cells": int(len(grid["C"]) * len(grid["gamma"])), "grid_s": {},
                  "tail_share_modelled": {}}
        GridSearchSVC(grid, cv(), tol=G.TOL, backend=hip).fit(X, y)  # warm-up: code objects, allocator
        for order in JOB_ORDERS:
            best = None
            for _ in range(3):
                search, s = timed(lambda: GridSearchSVC(grid, cv(), tol=G.TOL, backend=hip, job_order=order).fit(X, y))
                best = s if best is None else min(best, s)
            result["grid_s"][order] = round(best, 4)
            it = search.n_iter_  # [split, gamma, C, pair]
            per_split = []
            for sp in range(it.shape[0]):
                flat = it[sp].reshape(-1).astype(np.int64)
                if order == "c_desc":
                    c = np.broadcast_to(np.arange(it.shape[2])[None, :, None], it[sp].shape).reshape(-1)
                    flat = flat[np.argsort(-c, kind="stable")]  # largest C first (the pair-length key left out of the model)
                per_split.append(tail_share(flat))
            result["tail_share_modelled"][order] = round(float(np.mean(per_split)), 3)
        it = search.n_iter_.reshape(-1)
        result["jobs"] = int(it.size)
        result["iterations"] = {"min": int(it.min()), "median": float(np.median(it)), "max": int(it.max()),
                                "sum": int(it.sum())}
        result["best"] = {"params": search.best_params_, "score": search.best_score_}
        tb = TimedBackend(hip)
        GridSearchSVC(grid, cv(), tol=G.TOL, backend=tb).fit(X, y)
        rows = {}
        for name, _, us in tb.log:
            r = rows.setdefault(name, {"launches": 0, "us": 0.0})
            r["launches"] += 1
            r["us"] = round(r["us"] + us, 1)
        result["launches"] = rows
        if args.loop:
            splits = list(cv().split(X, y))

            def loop():
                counts = []
                for train, test in splits:
                    for C in grid["C"]:
                        for gamma in grid["gamma"]:
                            m = SVC(kernel="rbf", gamma=float(gamma), C=float(C), tol=G.TOL, backend=hip).fit(X[train], y[train])
                            counts.append(int((m.predict(X[test]) == y[test]).sum()))
                return counts
            _, s = timed(loop)
            result["loop_s"] = round(s, 3)
            result["ratio"] = round(s / min(result["grid_s"].values()), 2)
        if args.sklearn:
            try:
                from sklearn.model_selection import GridSearchCV, StratifiedShuffleSplit as SkSplit
                from sklearn.svm import SVC as SK
            except ImportError:
                SK = None
            if SK is not None:
                t0 = time.perf_counter()
                GridSearchCV(SK(), grid, cv=SkSplit(n_splits=G.N_SPLITS, test_size=G.TEST_SIZE, random_state=G.SEED)).fit(X, y)
                result["sklearn_cpu_s"] = round(time.perf_counter() - t0, 2)
        print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
