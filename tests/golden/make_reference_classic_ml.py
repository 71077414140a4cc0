"""Writes tests/golden/reference_classic_ml.{json,npz}: scikit-learn's SVC -- the estimator the reference calls
(classify/classic_ml_trainer.py:48-49,52-54,105), unchanged -- executed on SyntheticDataLoader scenes.  Needs
scikit-learn (present on the build machine only); the tests read the two files and never run this script.

    python tests/golden/make_reference_classic_ml.py

Inputs are not stored: tests/svm_cases.py re-makes them from the loader's seeded numpy.random.RandomState.  Per case:
the model at tol = 1e-6 (support_, n_support_, dual_coef_, intercept_), the float64 dual objective of every pair,
decision_function / predict on the validation rows, predict on the whole scene, OA / AA / kappa / confusion matrix
from sklearn.metrics, and the yardsticks measured on scikit-learn alone:
  delta_ref      max |decision(tol 1e-3) - decision(tol 1e-6)| on the validation rows
  obj_margin     2 x max relative difference of the pair objectives between tol 1e-3 and tol 1e-6
  unstable_*     rows whose vote does not survive handing every |dec| <= 2 delta_ref to the winner's opponents
                 (asserted here: at most 3 % of the rows of any case)
  emu_n_iter_max iterations the emulation of the product's solver (tests/emu_svm.py) needs for its slowest pair."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from sklearn.metrics import accuracy_score, balanced_accuracy_score, cohen_kappa_score, confusion_matrix  # noqa: E402
from sklearn.svm import SVC  # noqa: E402

from tests import svm_cases as S  # noqa: E402


def main():
    meta, arrays = {"sklearn": __import__("sklearn").__version__, "tol": S.TOL, "cases": {}}, {}
    for case in S.CASES:
        X, y, Xv, yv, _ = S.load_case_data(case)
        scene, (h, w) = S.load_scene_rows(case)
        args = S.svc_args(case)
        fine = SVC(tol=S.TOL, cache_size=1000, decision_function_shape="ovo", **args).fit(X, y)
        coarse = SVC(tol=1e-3, cache_size=1000, decision_function_shape="ovo", **args).fit(X, y)
        n_cls = len(fine.classes_)
        gamma = S.gamma_value(case, X)
        dec, dec_coarse = fine.decision_function(Xv), coarse.decision_function(Xv)
        delta_ref = float(np.abs(dec - dec_coarse).max())
        obj = S.pair_objectives(fine.dual_coef_, fine.n_support_, _k_sv(case, X, fine, gamma))
        obj_c = S.pair_objectives(coarse.dual_coef_, coarse.n_support_, _k_sv(case, X, coarse, gamma))
        obj_margin = 2.0 * float(np.max(np.abs(obj_c - obj) / np.abs(obj)))
        pred_v, pred_s = fine.predict(Xv), fine.predict(scene)
        delta = 2.0 * delta_ref
        un_v = S.unstable_mask(S.ovo_decisions(dec, n_cls), np.searchsorted(fine.classes_, pred_v), delta)
        un_s = S.unstable_mask(S.ovo_decisions(fine.decision_function(scene), n_cls),
                               np.searchsorted(fine.classes_, pred_s), delta)
        assert un_v.mean() <= 0.03 and un_s.mean() <= 0.03, (case, un_v.mean(), un_s.mean())
        # the product's solver on the same problem, emulated: iteration counts for the cap of hypel_svm_smo_ovo
        from tests.emu_backend import EmuBackend
        import tests.emu_svm  # noqa: F401
        from hypelcnn_amd.classic.svc import SVC as Product
        emu = Product(tol=S.TOL, backend=EmuBackend(), **args).fit(X, y)
        marginal = np.array([int((np.abs(fine.dual_coef_[:, s0:s0 + n]).max(0) <= delta).sum()) for s0, n in
                             zip(np.concatenate([[0], np.cumsum(fine.n_support_)[:-1]]), fine.n_support_)])
        meta["cases"][case] = dict(
            CASES=S.CASES[case], gamma=gamma, delta_ref=delta_ref, obj_margin=obj_margin,
            unstable_share_validation=float(un_v.mean()), unstable_share_scene=float(un_s.mean()),
            sklearn_n_iter_max=int(fine.n_iter_.max()), emu_n_iter_max=int(emu.n_iter_.max()),
            emu_n_iter_sum=int(emu.n_iter_.sum()), scene_shape=[h, w],
            oa=float(accuracy_score(yv, pred_v)), aa=float(balanced_accuracy_score(yv, pred_v)),
            kappa=float(cohen_kappa_score(yv, pred_v)))
        put = lambda k, v: arrays.__setitem__(f"{case}/{k}", v)  # noqa: E731
        put("support", fine.support_.astype(np.int32))
        put("n_support", fine.n_support_.astype(np.int32))
        put("dual_coef", fine.dual_coef_)
        put("intercept", fine.intercept_)
        put("objective", obj)
        put("decision", dec.astype(np.float32))
        put("predict_validation", pred_v.astype(np.uint8))
        put("predict_scene", pred_s.astype(np.uint8))
        put("unstable_validation", np.packbits(un_v))
        put("unstable_scene", np.packbits(un_s))
        put("n_marginal", marginal.astype(np.int32))
        put("confusion", confusion_matrix(yv, pred_v).astype(np.int64))
        if case == "small_rbf":
            order = np.argsort(y, kind="stable")
            put("K", S.kernel64(case, X[order], X[order], gamma))  # float64, rows sorted by class
        print(case, json.dumps(meta["cases"][case]))
    with open(S.JSON_PATH, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    np.savez_compressed(S.NPZ_PATH, **arrays)
    print(os.path.getsize(S.JSON_PATH), os.path.getsize(S.NPZ_PATH))


def _k_sv(case, X, model, gamma):
    """float64 kernel matrix of a model's support vectors"""
    return S.kernel64(case, X[model.support_], X[model.support_], gamma)


if __name__ == "__main__":
    main()
