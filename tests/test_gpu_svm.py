"""-m gpu: the support-vector kernels (csrc/svm.hip) and hypelcnn_amd.classic.svc on the device, held to scikit-learn's
outputs in tests/golden/reference_classic_ml.{json,npz} under the contract of tests/svm_cases.py: per-pair dual
objective within obj_margin, decisions within 2 x delta_ref, stable labels exact with at most 3 % of the rows left
out, support counts within the marginal vectors, the set at the bound C.  Every bound comes from scikit-learn's own
tol 1e-3 vs 1e-6 spread, stored by tests/golden/make_reference_classic_ml.py; none from the code under test."""
import os

import numpy as np
import pytest
import torch

import tests.emu_svm as E
from hypelcnn_amd.backend import Ref, SVM_PAIR_DTYPE
from hypelcnn_amd.classic import svc as P
from hypelcnn_amd.classify import classic_ml_trainer as T
from tests import svm_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def fixture():
    return S.load_fixture()


_models = {}


def _model(case, hip):
    if case not in _models:
        X, y = S.load_case_data(case)[:2]
        _models[case] = P.SVC(tol=S.TOL, backend=hip, **S.svc_args(case)).fit(X, y)
    return _models[case]


@pytest.mark.parametrize("kind,degree", [(E.RBF, 3), (E.POLY, 1), (E.POLY, 3)])
@pytest.mark.parametrize("rows,cols,ld", [(37, 53, 56), (130, 64, 64), (5, 7, 7)])
def test_kernel_apply_vs_float64(hip, kind, degree, rows, cols, ld):
    """Stored fp32 values of a float64 evaluation: half an ulp of the value + the fp64 library's exp."""
    rng = np.random.default_rng(rows * 1000 + cols)
    x, z = rng.standard_normal((rows, 9)) * 3e3, rng.standard_normal((cols, 9)) * 3e3
    g = np.zeros((rows, ld), np.float32)
    g[:, :cols] = x @ z.T
    rn, cn = (x * x).sum(1), (z * z).sum(1)
    gamma, coef0 = (1e-8, 0.0) if kind == E.RBF else (3e-8, 0.5)
    want = E.kernel_values(g[:, :cols], kind, gamma, coef0, degree, rn, cn)
    gd, rnd, cnd = (torch.from_numpy(a.reshape(-1).copy()).to(hip.device) for a in (g, rn, cn))
    hip.call("svm_kernel_apply_f32", Ref(gd), ld, rows, cols, kind, gamma, coef0, degree, Ref(rnd), Ref(cnd))
    got = gd.cpu().numpy().reshape(rows, ld)
    err = np.abs(got[:, :cols] - want) / np.maximum(np.abs(want), 1e-30)
    print("kernel_apply max rel err", err.max())
    assert err.max() <= 2.0 ** -23
    assert np.array_equal(got[:, cols:], g[:, cols:])  # pad columns untouched


def test_center_norms_vs_float64(hip):
    rng = np.random.default_rng(3)
    for rows, cols, ld in [(19, 3625, 3628), (7, 10, 10), (3, 5, 8)]:
        x = np.zeros((rows, ld), np.float32)
        x[:, :cols] = 2500 + 900 * rng.standard_normal((rows, cols))
        mean = x[:, :cols].astype(np.float64).mean(0).astype(np.float32)
        xd, md = torch.from_numpy(x.reshape(-1).copy()).to(hip.device), torch.from_numpy(mean).to(hip.device)
        nd = torch.zeros(rows, dtype=torch.float64, device=hip.device)
        hip.call("svm_center_norms_f32", Ref(xd), ld, rows, cols, Ref(md), Ref(nd))
        got = xd.cpu().numpy().reshape(rows, ld)
        want = x[:, :cols] - mean
        assert np.array_equal(got[:, :cols], want) and np.array_equal(got[:, cols:], x[:, cols:])
        ref = (want.astype(np.float64) ** 2).sum(1)
        assert np.abs(nd.cpu().numpy() - ref).max() <= 1e-12 * ref.max()


def test_vote_bit_exact_on_crafted_ties(hip):
    rng = np.random.default_rng(5)
    for n_cls in (2, 3, 15, 40):
        n_pairs = n_cls * (n_cls - 1) // 2
        ld, rows = n_pairs + 3, 700
        dec = rng.choice(np.float32([-1, 0, 0.0, 1, -0.0, 1e-30, np.nan]), size=(rows, ld))  # ties and dec == 0 abound
        dd = torch.from_numpy(dec.reshape(-1).copy()).to(hip.device)
        out = torch.zeros(rows, dtype=torch.uint8, device=hip.device)
        hip.call("svm_vote", Ref(dd), ld, rows, n_cls, None, None, Ref(out), 0)
        assert np.array_equal(out.cpu().numpy(), E.vote(dec, n_cls).astype(np.uint8))
    dec = np.float32([[1, -1, 1], [0, 0, 0], [-1, 1, 0]])  # one vote each -> 0; dec == 0 -> higher class -> 2; tie -> 0
    labels = torch.tensor([10, 20, 30], dtype=torch.uint8, device=hip.device)
    pts = torch.tensor([[2, 0], [0, 1], [1, 1]], dtype=torch.int32, device=hip.device).reshape(-1)
    raster = torch.full((6,), 255, dtype=torch.uint8, device=hip.device)
    hip.call("svm_vote", Ref(torch.from_numpy(dec.reshape(-1)).to(hip.device)), 3, 3, 3, Ref(labels), Ref(pts), Ref(raster), 3)
    assert raster.cpu().numpy().tolist() == [255, 255, 10, 30, 10, 255]


def test_smo_ovo_on_stored_K(hip, fixture):
    """The solver alone, on the float64 K the fixture script stored (rounded to fp32 here), vs its emulation twin and
    vs scikit-learn's objective."""
    meta, fx = fixture
    case = "small_rbf"
    K = fx[f"{case}/K"].astype(np.float32)
    y = S.load_case_data(case)[1]
    count = np.bincount(y)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    tab, total = P.pair_table(start, count)
    assert tab.dtype == SVM_PAIR_DTYPE
    l, n_pairs = len(K), len(tab)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(hip.device)  # noqa: E731
    kd, td = torch.from_numpy(K.reshape(-1)).to(hip.device), dev(tab)
    ay, rho, obj = (torch.zeros(n, dtype=torch.float64, device=hip.device) for n in (total, n_pairs, n_pairs))
    it, st = (torch.zeros(n_pairs, dtype=torch.int32, device=hip.device) for _ in range(2))
    C = S.CASES[case]["C"]
    hip.call("svm_smo_ovo", Ref(kd), l, Ref(td), n_pairs, int((tab["na"] + tab["nb"]).max()), C, S.TOL, P.DEFAULT_MAX_ITER,
             Ref(ay), Ref(rho), Ref(obj), Ref(it), Ref(st), None)
    hip.synchronize()
    assert (st.cpu().numpy() == 0).all()
    m = meta["cases"][case]
    for p, rec in enumerate(tab):
        a0, na, b0, nb, off = (int(rec[f]) for f in ("a0", "na", "b0", "nb", "out_off"))
        rows = np.concatenate([np.arange(a0, a0 + na), np.arange(b0, b0 + nb)])
        v = ay.cpu().numpy()[off:off + na + nb]
        K64 = fx[f"{case}/K"][np.ix_(rows, rows)]
        o64 = 0.5 * v @ K64 @ v - np.abs(v).sum()
        ref = fx[f"{case}/objective"][p]
        print(f"pair {p}: iterations {int(it[p])}, objective {o64:.9e} (fixture {ref:.9e}), rho {float(rho[p]):.6e}")
        assert (o64 - ref) / abs(ref) <= m["obj_margin"]
        assert abs(float(obj[p]) - o64) <= 1e-5 * abs(o64)  # the solver's own figure (from its fp32 K)
        assert abs(-float(rho[p]) - fx[f"{case}/intercept"][p]) <= 2 * m["delta_ref"]
        assert np.all(np.abs(v) <= C) and abs(v.sum()) <= 1e-9 * C * len(v)  # box and equality constraint


@pytest.mark.parametrize("case", list(S.CASES))
def test_fit_matches_libsvm(case, hip, fixture):
    meta, fx = fixture
    model = _model(case, hip)
    print(f"{case}: iterations max {int(model.n_iter_.max())} sum {int(model.n_iter_.sum())}")
    S.check_fit(model, case, meta, fx)
    assert model.dual_coef_.shape[0] == len(model.classes_) - 1
    assert np.abs(model.intercept_ - fx[f"{case}/intercept"]).max() <= 2 * meta["cases"][case]["delta_ref"]


@pytest.mark.parametrize("case", ["grss2013_rbf_clip", "grss2013_poly"])
def test_fit_bound_set(case, hip, fixture):
    at_bound, nonzero = S.check_bound_set(_model(case, hip), case, fixture[1])
    if case == "grss2013_poly":  # the case that does clip on this scene
        assert at_bound > nonzero / 3


@pytest.mark.parametrize("case", list(S.CASES))
def test_predict_matches_fixture_labels(case, hip, fixture):
    meta, fx = fixture
    model = _model(case, hip)
    S.check_labels(model.predict(S.load_case_data(case)[2]), case, "validation", fx)
    scene, _ = S.load_scene_rows(case)
    S.check_labels(model.predict(torch.from_numpy(scene).to(hip.device)), case, "scene", fx)  # a device tensor as X


def test_chunked_prediction_identical(hip):
    model = _model("grss2013_rbf", hip)
    Xv = S.load_case_data("grss2013_rbf")[2]
    outs = []
    for chunk in (64, 150, None):
        model.chunk_rows = chunk
        outs.append((model.predict(Xv), model.decision_function(Xv)))
    model.chunk_rows = None
    for lab, dec in outs[1:]:
        assert np.array_equal(lab, outs[0][0]) and np.array_equal(dec, outs[0][1])


def test_classic_ml_trainer_fullscene(hip, fixture, tmp_path):
    meta, fx = fixture
    case = "grss2013_rbf"
    out = T.main(["--loader_name", "SyntheticDataLoader", "--path", "grss2013", "--neighborhood", "2", "--fullscene",
                  "--base_log_path", str(tmp_path / "log"), "--output_path", str(tmp_path / "out"),
                  "--svc_tol", str(S.TOL)], backend=hip)
    _, predicted, cm, (oa, aa, kappa), scene = out[0]
    S.check_labels(predicted, case, "validation", fx)
    S.check_labels(scene, case, "scene", fx)
    if np.array_equal(predicted, fx[f"{case}/predict_validation"]):
        m = meta["cases"][case]
        assert np.array_equal(cm, fx[f"{case}/confusion"])
        assert max(abs(oa - m["oa"]), abs(aa - m["aa"]), abs(kappa - m["kappa"])) <= 1e-12
    from hypelcnn_amd.common.tiff_io import imread
    assert np.array_equal(imread(str(tmp_path / "out" / "result_raw.tif")), scene)
    assert os.path.exists(tmp_path / "log" / "metrics_SyntheticDataLoader_run0.txt")
