"""Writes tests/golden/reference_svm_grid.{json,npz}: scikit-learn's GridSearchCV, StratifiedShuffleSplit and SVC -- what
the reference's perform_hyperparamopt calls (classify/classic_ml_trainer.py:126-136), unchanged -- executed on
SyntheticDataLoader scenes.  Needs scikit-learn (present on the build machine only); the tests read the two files and
never run this script.

    python tests/golden/make_reference_svm_grid.py

Inputs are not stored (tests/svm_grid_cases.py re-makes them from the seeded loader).  Per case: the split indices, the
grid in ParameterGrid order, GridSearchCV's split / mean scores, ranks and best cell, and per split and cell from a
fit of SVC(C, gamma) at tol 1e-3 and one at 1e-6: n_correct at 1e-3, the test rows whose vote is unstable
(svm_cases.unstable_mask on the 1e-3 decisions, delta = 2 max |dec(1e-3) - dec(1e-6)| of that cell), scikit-learn's
iteration maximum (per-cell arrays in the npz, their overall maxima in the JSON).  Asserted here on scikit-learn alone: unstable (row, cell) entries <= 3 % of a case's entries.  The
product's solver is then run on the emulation (tests/emu_svm_grid.py) for its per-cell iteration maxima; for the
grss2013 case they must stay at or below DEFAULT_MAX_ITER / 100.  Label vectors of svm_grid_cases.SPLIT_CASES: labels
are re-made by the tests, only scikit-learn's indices are stored."""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from joblib import Parallel, delayed  # noqa: E402
from sklearn.model_selection import GridSearchCV, StratifiedShuffleSplit  # noqa: E402
from sklearn.svm import SVC  # noqa: E402

from tests import svm_cases as S  # noqa: E402
from tests import svm_grid_cases as G  # noqa: E402

JOBS = 8
CONSTANT_KERNEL_GAMMA = 1.0  # from here up every off-diagonal kernel value of these scenes is 0: dec = -rho


def one_cell(X, y, train, test, C, gamma):
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (in the worker process) a ConvergenceWarning would be an unconverged cell
        coarse = SVC(C=C, gamma=gamma, tol=G.TOL, cache_size=500, decision_function_shape="ovo").fit(X[train], y[train])
        fine = SVC(C=C, gamma=gamma, tol=1e-6, cache_size=500, decision_function_shape="ovo").fit(X[train], y[train])
    n_cls = len(coarse.classes_)
    dec = S.ovo_decisions(coarse.decision_function(X[test]), n_cls)
    delta = 2.0 * float(np.abs(dec - S.ovo_decisions(fine.decision_function(X[test]), n_cls)).max())
    pred = coarse.predict(X[test])
    un = S.unstable_mask(dec, np.searchsorted(coarse.classes_, pred), delta)
    rho_min = float(np.abs(coarse.intercept_).min())
    return int((pred == y[test]).sum()), un, int(coarse.n_iter_.max()), delta, rho_min


def main():
    import sklearn
    meta = {"sklearn": sklearn.__version__, "numpy": np.__version__, "tol": G.TOL, "n_splits": G.N_SPLITS,
            "test_size": G.TEST_SIZE, "random_state": G.SEED, "cases": {},
            "choice": "grss2013: the only timing of the full synthetic scene (2159 rows x 3625 features, 15 classes) is "
                      "that one split of the 13 x 13 grid had not finished its first 13 cells after 20 minutes in "
                      "scikit-learn, i.e. more than 1.5 minutes per fit; a 5 x 5 window needs 2 splits x 25 cells x 2 "
                      "tolerances = 100 such fits plus GridSearchCV's 50, beyond the 15 minutes this script may take "
                      "even on 8 processes.  So the scene is shrunk with the loader's own options "
                      "to h=30:w=40 (539 rows, splits 485 / 54) and the grid is the 5 x 5 window C 1e-2..1e2, gamma "
                      "1e-9..1e-5 of the reference's 13 x 13: the window that holds the reference's own gamma for this "
                      "sensor (1e-9) and its neighbours, at the C values whose pairs converge within "
                      "DEFAULT_MAX_ITER / 100 iterations in the emulation (asserted below)."}
    arrays = {}
    for key, (labels, n_splits, test_size, seed) in G.SPLIT_CASES.items():
        cv = StratifiedShuffleSplit(n_splits=n_splits, test_size=test_size, random_state=seed)
        for s, (train, test) in enumerate(cv.split(np.zeros((len(labels), 1)), labels)):
            arrays[f"splits/{key}/train{s}"], arrays[f"splits/{key}/test{s}"] = train.astype(np.int32), test.astype(np.int32)
    for case in G.CASES:
        t0 = time.time()
        X, y = G.load_case_data(case)
        grid = G.grid_of(case)
        cells = [(float(c), float(g)) for c in grid["C"] for g in grid["gamma"]]
        cv = StratifiedShuffleSplit(n_splits=G.N_SPLITS, test_size=G.TEST_SIZE, random_state=G.SEED)
        splits = list(cv.split(X, y))
        out = Parallel(n_jobs=JOBS)(delayed(one_cell)(X, y, tr, te, c, g) for tr, te in splits for c, g in cells)
        n_test = len(splits[0][1])
        shape = (G.N_SPLITS, len(cells), n_test)
        n_correct = np.array([o[0] for o in out], np.int32).reshape(shape[:2])
        unstable = np.stack([o[1] for o in out]).reshape(shape)
        sk_iter = np.array([o[2] for o in out], np.int64).reshape(shape[:2])
        delta = np.array([o[3] for o in out]).reshape(shape[:2])
        rho_min = np.array([o[4] for o in out]).reshape(shape[:2])
        share = float(unstable.mean())
        assert share <= 0.03, (case, share)  # the cap: change the scene, not the cap
        const = np.array([g >= CONSTANT_KERNEL_GAMMA for _, g in cells])
        rho_near_zero = int((rho_min[:, const] <= delta[:, const]).sum())
        assert rho_near_zero == 0, (case, rho_near_zero)  # such a cell decides by the sign of a rounding: change the scene
        gs = GridSearchCV(SVC(), grid, cv=cv, n_jobs=JOBS, error_score="raise").fit(X, y)  # (no max_iter: it converges)
        res = gs.cv_results_
        assert [(p["C"], p["gamma"]) for p in res["params"]] == cells
        for s in range(G.N_SPLITS):
            assert np.array_equal(res[f"split{s}_test_score"], n_correct[s] / n_test)
        # the product on the emulation: iteration counts of its solver per cell
        from tests.emu_backend import EmuBackend
        import tests.emu_svm  # noqa: F401
        import tests.emu_svm_grid  # noqa: F401
        from hypelcnn_amd.classic.model_selection import GridSearchSVC, StratifiedShuffleSplit as ProductSplit
        from hypelcnn_amd.classic.svc import DEFAULT_MAX_ITER
        emu = GridSearchSVC(grid, ProductSplit(G.N_SPLITS, G.TEST_SIZE, random_state=G.SEED), tol=G.TOL,
                            backend=EmuBackend()).fit(X, y)
        emu_iter = np.stack([emu.cv_results_[f"split{s}_n_iter_max"] for s in range(G.N_SPLITS)])
        if case == "grss2013":
            assert emu_iter.max() <= DEFAULT_MAX_ITER // 100, emu_iter.max()
        meta["cases"][case] = dict(
            path=G.CASES[case]["path"], C_decades=list(G.CASES[case]["C"]), gamma_decades=list(G.CASES[case]["gamma"]),
            n_rows=int(len(y)), n_train=int(len(splits[0][0])), n_test=int(n_test), class_counts=np.bincount(y).tolist(),
            unstable_share=share, unstable_entries=int(unstable.sum()), constant_kernel_cells_rho_within_delta=rho_near_zero,
            sklearn_n_iter_max_overall=int(sk_iter.max()), emu_n_iter_max_overall=int(emu_iter.max()),
            best_index=int(gs.best_index_), best_params={k: float(v) for k, v in gs.best_params_.items()},
            best_score=float(gs.best_score_), seconds=round(time.time() - t0, 1))
        put = lambda k, v: arrays.__setitem__(f"{case}/{k}", v)  # noqa: E731
        for s, (train, test) in enumerate(splits):
            put(f"train{s}", train.astype(np.int32))
            put(f"test{s}", test.astype(np.int32))
            put(f"split{s}_test_score", res[f"split{s}_test_score"])
        put("n_correct", n_correct)
        put("unstable", np.packbits(unstable))
        put("unstable_shape", np.array(shape, np.int64))
        put("delta", delta)
        put("sklearn_n_iter_max", sk_iter.astype(np.int32))  # [split, cell]
        put("emu_n_iter_max", emu_iter.astype(np.int32))
        put("param_C", np.array([c for c, _ in cells]))
        put("param_gamma", np.array([g for _, g in cells]))
        put("mean_test_score", res["mean_test_score"])
        put("rank_test_score", res["rank_test_score"].astype(np.int32))
        print(case, json.dumps(meta["cases"][case]), flush=True)
    with open(G.JSON_PATH, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    np.savez_compressed(G.NPZ_PATH, **arrays)
    print(os.path.getsize(G.JSON_PATH), os.path.getsize(G.NPZ_PATH))


if __name__ == "__main__":
    main()
