"""CPU: hypelcnn_amd.classic.svc and classify/classic_ml_trainer.py on the numpy twin of the hypel_svm_* entry points
(tests/emu_svm.py), held to scikit-learn's outputs in tests/golden/reference_classic_ml.{json,npz}
(tests/golden/make_reference_classic_ml.py; contract in tests/svm_cases.py)."""
import os

import numpy as np
import pytest

import tests.emu_svm as E
from hypelcnn_amd.classic import svc as P
from hypelcnn_amd.classify import classic_ml_trainer as T
from tests import svm_cases as S
from tests.emu_backend import EmuBackend


@pytest.fixture(scope="module")
def fixture():
    return S.load_fixture()


def _fit(case, **kw):
    X, y = S.load_case_data(case)[:2]
    return P.SVC(tol=S.TOL, backend=EmuBackend(), **S.svc_args(case), **kw).fit(X, y)


@pytest.mark.parametrize("case", ["small_rbf", "avon_rbf", "grss2013_poly"])
def test_emu_fit_matches_libsvm(case, fixture):
    meta, fx = fixture
    model = _fit(case)
    S.check_fit(model, case, meta, fx)
    assert np.array_equal(model.classes_, np.unique(S.load_case_data(case)[1]))
    assert model.dual_coef_.shape == fx[f"{case}/dual_coef"].shape
    assert np.abs(model.intercept_ - fx[f"{case}/intercept"]).max() <= 2 * meta["cases"][case]["delta_ref"]
    Xv = S.load_case_data(case)[2]
    S.check_labels(model.predict(Xv), case, "validation", fx)
    assert model.n_iter_.max() <= meta["cases"][case]["emu_n_iter_max"]  # what the cap of svc.py is derived from


def test_emu_bound_set_on_the_clipping_case(fixture):
    at_bound, nonzero = S.check_bound_set(_fit("grss2013_poly"), "grss2013_poly", fixture[1])
    assert at_bound > nonzero / 3


def test_iteration_cap_margin(fixture):
    worst = max(c["emu_n_iter_max"] for c in fixture[0]["cases"].values())
    assert P.DEFAULT_MAX_ITER == 100 * worst and P.DEFAULT_MAX_ITER <= P.SVM_MAX_ITER_LIMIT


def test_kernel_matrix_matches_stored_K(fixture):
    """kernel_apply twin on float64 products vs the K the fixture script stored (rows sorted by class)."""
    _, fx = fixture
    X, y = S.load_case_data("small_rbf")[:2]
    Z = X[np.argsort(y, kind="stable")].astype(np.float32)
    Z = Z - Z.astype(np.float64).mean(0).astype(np.float32)
    n2 = (Z.astype(np.float64) ** 2).sum(1)
    K = E.kernel_values(Z.astype(np.float64) @ Z.astype(np.float64).T, E.RBF, 1e-8, 0.0, 3, n2, n2)
    assert np.abs(K - fx["small_rbf/K"]).max() < 1e-6


def test_bookkeeping_pair_table_and_packing():
    start, count = np.array([0, 3, 5]), np.array([3, 2, 4])
    tab, total = P.pair_table(start, count)
    assert total == 5 + 7 + 6 and tab["out_off"].tolist() == [0, 5, 12]
    assert [(int(r["a0"]), int(r["na"]), int(r["b0"]), int(r["nb"])) for r in tab] == [(0, 3, 3, 2), (0, 3, 5, 4), (3, 2, 5, 4)]
    ay = np.zeros(total)
    ay[0], ay[3] = 2.0, -2.0          # pair (0,1): row 0 (class 0) and row 3 (class 1)
    ay[5 + 1], ay[5 + 3] = 1.5, -1.5  # pair (0,2): row 1 (class 0) and row 5 (class 2)
    ay[12 + 0], ay[12 + 2] = 0.5, -0.5  # pair (1,2): row 3 (class 1) and row 5 (class 2)
    sv, n_support, dual, coef = P.pack_model(ay, tab, start, count)
    assert sv.tolist() == [0, 1, 3, 5] and n_support.tolist() == [2, 1, 1]
    # libsvm: a class-c vector holds its coefficient against class o in row o (o < c) or o - 1 (o > c)
    assert dual.tolist() == [[2.0, 0.0, -2.0, -1.5], [0.0, 1.5, 0.5, -0.5]]
    assert coef[:, 0].tolist() == [2.0, 0, -2.0, 0] and coef[:, 2].tolist() == [0, 0, 0.5, -0.5]


def test_rho_sign_and_two_class_flip(fixture):
    meta, fx = fixture
    model = _fit("avon_rbf")
    assert model.dual_coef_.shape[0] == 1 and model.decision_function(S.load_case_data("avon_rbf")[2]).ndim == 1
    assert np.allclose(model.intercept_, model._rho)  # binary: scikit-learn's flip of -rho
    assert np.abs(model.intercept_ - fx["avon_rbf/intercept"]).max() <= 2 * meta["cases"]["avon_rbf"]["delta_ref"]


def test_vote_rule_ties_and_zero():
    dec = np.zeros((3, 3), np.float32)        # pairs (0,1), (0,2), (1,2)
    dec[0] = [1, -1, 1]                       # 0, 2, 1 -> one vote each: first class with the maximum = 0
    dec[1] = [0, 0, 0]                        # dec == 0 votes for the HIGHER class: 1, 2, 2 -> 2
    dec[2] = [-1, 1, 0]                       # 1, 0, 2 -> tie -> 0
    assert E.vote(dec, 3).tolist() == [0, 2, 0]


def test_iteration_cap_reports_not_converged():
    X, y = S.load_case_data("small_rbf")[:2]
    with pytest.raises(P.NotConvergedError, match="not converged after max_iter=5"):
        P.SVC(tol=S.TOL, backend=EmuBackend(), max_iter=5, **S.svc_args("small_rbf")).fit(X, y)


def test_refusals():
    with pytest.raises(NotImplementedError, match="rbf.*poly"):
        P.SVC(kernel="sigmoid")
    with pytest.raises(NotImplementedError, match="degree 1..3"):
        P.SVC(kernel="poly", degree=4)
    with pytest.raises(ValueError, match="bounded"):
        P.SVC(max_iter=P.SVM_MAX_ITER_LIMIT + 1)
    with pytest.raises(ValueError, match="at most 255 classes"):
        P.SVC(backend=EmuBackend()).fit(np.zeros((300, 2), np.float32), np.arange(300))
    with pytest.raises(NotImplementedError, match="RandomForestClassifier"):
        T.main(["--estimator", "RandomForestClassifier", "--loader_name", "SyntheticDataLoader",
                "--path", S.CASES["small_rbf"]["path"], "--neighborhood", "2"], backend=EmuBackend())
    with pytest.raises(NotImplementedError, match="hyperparamopt"):
        T.main(["--hyperparamopt"], backend=EmuBackend())


def test_cli_end_to_end_on_emulation(tmp_path, fixture):
    meta, fx = fixture
    case = "small_rbf"
    c = S.CASES[case]
    out = T.main(["--loader_name", "SyntheticDataLoader", "--path", c["path"], "--neighborhood", "2",
                  "--base_log_path", str(tmp_path / "log"), "--output_path", str(tmp_path / "out"), "--fullscene",
                  "--svc_gamma", str(c["gamma"]), "--svc_c", str(c["C"]), "--svc_tol", str(S.TOL)], backend=EmuBackend())
    _, predicted, cm, (oa, aa, kappa), scene = out[0]
    m = meta["cases"][case]
    S.check_labels(predicted, case, "validation", fx)
    S.check_labels(scene, case, "scene", fx)
    # 5. metrics: the fixture's are sklearn.metrics on scikit-learn's labels; equal labels -> equal integers, floats 1e-12
    if np.array_equal(predicted, fx[f"{case}/predict_validation"]):
        assert np.array_equal(cm, fx[f"{case}/confusion"])
        assert max(abs(oa - m["oa"]), abs(aa - m["aa"]), abs(kappa - m["kappa"])) <= 1e-12
    log = tmp_path / "log"
    assert np.array_equal(np.loadtxt(log / "confusion_matrix_SyntheticDataLoader_run0.csv", delimiter=",", ndmin=2), cm)
    lines = (log / "metrics_SyntheticDataLoader_run0.txt").read_text().split("\n")
    assert lines[0] == "OA,AA,KAPPA" and lines[1] == "%.6f,%.6f,%.6f" % (oa, aa, kappa)
    assert os.path.exists(log / "params_SyntheticDataLoader_run0.json")
    from hypelcnn_amd.common.tiff_io import imread
    assert np.array_equal(imread(str(tmp_path / "out" / "result_raw.tif")), scene)
    assert imread(str(tmp_path / "out" / "result_colorized.tif")).shape == scene.shape + (3,)


@pytest.mark.parametrize("case", list(S.CASES))
def test_host_metrics_equal_sklearn_metrics(case, fixture):
    """OA / AA / kappa / confusion matrix of the host code on the FIXTURE's labels vs sklearn.metrics' stored values."""
    meta, fx = fixture
    yv = S.load_case_data(case)[3]
    cm = T.confusion_matrix(yv, fx[f"{case}/predict_validation"])
    assert np.array_equal(cm, fx[f"{case}/confusion"])
    oa, aa, kappa = T.scores(cm)
    m = meta["cases"][case]
    assert max(abs(oa - m["oa"]), abs(aa - m["aa"]), abs(kappa - m["kappa"])) <= 1e-12
