"""CPU: hypelcnn_amd.classic.model_selection and the --svc_grid flags of classify/classic_ml_trainer.py on the numpy
twins of the grid-search entry points (tests/emu_svm_grid.py), held to scikit-learn's GridSearchCV /
StratifiedShuffleSplit / SVC outputs in tests/golden/reference_svm_grid.{json,npz}
(tests/golden/make_reference_svm_grid.py; contract in tests/svm_grid_cases.py)."""
import json
import warnings

import numpy as np
import pytest
import torch

import tests.emu_svm as E
import tests.emu_svm_grid as EG
from hypelcnn_amd.backend import Ref, SVM_JOB_DTYPE
from hypelcnn_amd.classic import model_selection as M
from hypelcnn_amd.classic import svc as P
from hypelcnn_amd.classify import classic_ml_trainer as T
from tests import svm_grid_cases as G
from tests.emu_backend import EmuBackend


@pytest.fixture(scope="module")
def fixture():
    return G.load_fixture()


def _cv():
    return M.StratifiedShuffleSplit(n_splits=G.N_SPLITS, test_size=G.TEST_SIZE, random_state=G.SEED)


# ---- 1. split indices ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.CASES))
def test_split_indices_equal_sklearn_on_the_cases(case, fixture):
    _, y = G.load_case_data(case)
    G.check_splits(M.StratifiedShuffleSplit, y, G.N_SPLITS, G.TEST_SIZE, G.SEED, fixture[1], case)


@pytest.mark.parametrize("key", list(G.SPLIT_CASES))
def test_split_indices_equal_sklearn_on_label_vectors(key, fixture):
    labels, n_splits, test_size, seed = G.SPLIT_CASES[key]
    G.check_splits(M.StratifiedShuffleSplit, labels, n_splits, test_size, seed, fixture[1], f"splits/{key}")


def test_splitter_refusals():
    with pytest.raises(NotImplementedError, match="test_size"):
        M.StratifiedShuffleSplit(n_splits=2, test_size=5, random_state=42)
    with pytest.raises(NotImplementedError, match="test_size"):
        M.StratifiedShuffleSplit(n_splits=2, random_state=42)
    with pytest.raises(NotImplementedError, match="train_size"):
        M.StratifiedShuffleSplit(n_splits=2, test_size=0.1, train_size=0.5, random_state=42)
    with pytest.raises(NotImplementedError, match="random_state"):
        M.StratifiedShuffleSplit(n_splits=2, test_size=0.1)
    with pytest.raises(ValueError, match="only 1 member"):
        list(M.StratifiedShuffleSplit(2, 0.1, random_state=1).split(None, np.array([0] * 20 + [1])))
    with pytest.raises(NotImplementedError, match="'C' and 'gamma'"):
        M.GridSearchSVC({"C": [1.0], "degree": [2]}, _cv())


# ---- 2. + 3. the search vs the fixture --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.CASES))
def test_grid_search_on_emulation_matches_sklearn(case, fixture):
    meta, fx = fixture
    X, y = G.load_case_data(case)
    search = M.GridSearchSVC(G.grid_of(case), _cv(), tol=G.TOL, backend=EmuBackend()).fit(X, y)
    it_max = G.check_search(search, case, meta, fx)
    assert search.n_splits_ == G.N_SPLITS
    assert it_max == meta["cases"][case]["emu_n_iter_max_overall"]
    if case == "grss2013":
        assert it_max <= P.DEFAULT_MAX_ITER // 100
    assert meta["cases"][case]["unstable_share"] <= 0.03


def test_rank_and_order_rules():
    assert M.min_rank([0.5, 0.9, np.nan, 0.9, 0.1]).tolist() == [3, 1, 5, 1, 4]
    assert M.min_rank([np.nan, np.nan]).tolist() == [1, 1]
    cells = M.parameter_grid({"C": [1, 10], "gamma": [0.1, 0.2, 0.3]})
    assert [(c["C"], c["gamma"]) for c in cells] == [(1, .1), (1, .2), (1, .3), (10, .1), (10, .2), (10, .3)]


# ---- 4. the smo_grid twin ---------------------------------------------------------------------------------------------
def test_smo_grid_twin_equals_smo_pair_bitwise():
    rng = np.random.default_rng(11)
    be = EmuBackend()
    l, ldk = 30, 32
    x = rng.standard_normal((l, 4))
    d2 = ((x[:, None] - x[None]) ** 2).sum(2)
    planes = np.zeros((2, l, ldk), np.float32)
    for p, gamma in enumerate((0.3, 2.0)):
        planes[p, :, :l] = np.exp(-gamma * d2)
    tab, total = P.pair_table(np.array([0, 9, 19]), np.array([9, 10, 11]))
    Cs = [0.5, 40.0]
    jobs = np.zeros((2, 2, len(tab)), SVM_JOB_DTYPE)
    for name in ("a0", "na", "b0", "nb"):
        jobs[name] = tab[name]
    jobs["out_off"] = (np.arange(4).reshape(2, 2, 1)) * total + tab["out_off"]
    jobs["k_off"] = np.arange(2).reshape(2, 1, 1) * l * ldk
    jobs["c"] = np.array(Cs).reshape(1, 2, 1)
    jobs = jobs.reshape(-1)
    n = len(jobs)
    order = rng.permutation(n).astype(np.int32)
    ay, rho, obj = (torch.zeros(k, dtype=torch.float64) for k in (4 * total, n, n))
    it, st = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    be.call("svm_smo_grid", Ref(torch.from_numpy(planes.reshape(-1))), ldk, Ref(be.upload(jobs)), Ref(be.upload(order)), n, 21,
            1e-3, 1000, Ref(ay), Ref(rho), Ref(obj), Ref(it), Ref(st), None)
    for j, rec in enumerate(jobs):
        rows, na, nb = EG.job_rows(rec)
        K = planes[j // (2 * len(tab))][np.ix_(rows, rows)]
        want = E.smo_pair(K, na, float(rec["c"]), 1e-3, 1000)
        off = int(rec["out_off"])
        assert np.array_equal(ay.numpy()[off:off + na + nb], want[0])
        assert (rho[j].item(), obj[j].item(), it[j].item(), st[j].item()) == want[1:]
    # scatter_coef + vote_score twins on the same jobs: cell ci of gamma 0
    npp = 32
    coef, bias = torch.zeros(l * 2 * npp), torch.zeros(2 * npp)
    be.call("svm_scatter_coef_f32", Ref(ay), Ref(rho), Ref(be.upload(tab)), len(tab), 2, total, l, npp, Ref(coef), 2 * npp,
            Ref(bias))
    w = coef.numpy().reshape(l, 2 * npp)
    for ci in range(2):
        for p, rec in enumerate(tab):
            rows, na, nb = EG.job_rows(rec)
            off = ci * total + int(rec["out_off"])
            col = np.zeros(l, np.float32)
            col[rows] = ay.numpy()[off:off + na + nb]
            assert np.array_equal(w[:, ci * npp + p], col) and bias[ci * npp + p] == np.float32(-rho[ci * 3 + p].item())
        assert not w[:, ci * npp + 3:(ci + 1) * npp].any()
    dec = (planes[0, :, :l] @ w + bias.numpy()).astype(np.float32)
    truth = np.repeat(np.arange(3), [9, 10, 11]).astype(np.int32)
    correct = torch.zeros(2, dtype=torch.int32)
    be.call("svm_vote_score", Ref(torch.from_numpy(dec.reshape(-1))), 2 * npp, l, 3, 2, npp, Ref(torch.from_numpy(truth)),
            Ref(correct))
    assert correct.tolist() == [int((E.vote(dec[:, ci * npp:ci * npp + 3], 3) == truth).sum()) for ci in range(2)]


# ---- 5. unconverged cells ---------------------------------------------------------------------------------------------
def test_unconverged_cells_are_nan_and_rank_last():
    """max_iter=5 on two tight, well separated clusters: the cell (C = 100, gamma = 1e-3) converges in 3 iterations, the
    other five need 8 to 37 and reach the cap."""
    rng = np.random.RandomState(0)
    y = np.repeat([0, 1], [20, 20])
    X = (np.where(y[:, None] == 0, -1.0, 1.0) * np.ones((40, 3)) + 0.01 * rng.standard_normal((40, 3))).astype(np.float32)
    grid = {"C": [1e-2, 1e2], "gamma": [1e-3, 0.5, 1e3]}
    search = M.GridSearchSVC(grid, _cv(), tol=G.TOL, max_iter=5, backend=EmuBackend())
    with pytest.warns(UserWarning, match="5 of 6 cells"):
        search.fit(X, y)
    res = search.cv_results_
    assert np.isnan(res["mean_test_score"]).tolist() == [True, True, True, False, True, True]
    assert res["rank_test_score"].tolist() == [2, 2, 2, 1, 2, 2] and search.best_index_ == 3
    assert search.best_params_ == {"C": 100.0, "gamma": 1e-3} and search.best_score_ == 1.0
    assert res["split0_not_converged"].tolist() == [1, 1, 1, 0, 1, 1] and res["split0_n_iter_max"].tolist() == [5, 5, 5, 3, 5, 5]
    with pytest.raises(P.NotConvergedError, match="every one of the 2 cells"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        M.GridSearchSVC({"C": [1e-2], "gamma": [0.5, 1e3]}, _cv(), tol=G.TOL, max_iter=5, backend=EmuBackend()).fit(X, y)


# ---- 6. CLI -------------------------------------------------------------------------------------------------------------
def test_cli_grid_search_on_emulation(tmp_path, capsys):
    path = G.CASES["small"]["path"]
    out = T.main(["--loader_name", "SyntheticDataLoader", "--path", path, "--neighborhood", "2",
                  "--base_log_path", str(tmp_path / "log"), "--svc_gamma", "1e-8", "--svc_c", "1e3",
                  "--svc_grid", "--svc_grid_c", "-1:2:4", "--svc_grid_gamma", "-9:-6:4"], backend=EmuBackend())
    estimator, predicted, cm, _, scene = out[0]  # the return tuple keeps its five items
    grid = estimator.grid_search_
    assert grid is T.last_grid_search and len(grid.cv_results_["params"]) == 16 and scene is None
    text = capsys.readouterr().out
    assert "The best parameters are %s with a score of %0.2f" % (grid.best_params_, grid.best_score_) in text
    saved = json.loads((tmp_path / "log" / "svc_grid_SyntheticDataLoader_run0.json").read_text())
    assert saved["best_params"] == grid.best_params_ and saved["best_index"] == grid.best_index_
    assert saved["rank_test_score"] == grid.cv_results_["rank_test_score"].tolist()
    assert saved["params"][1] == {"C": 0.1, "gamma": 1e-8} and len(saved["split1_test_score"]) == 16
    assert saved["unconverged_cells"] == []
    assert (tmp_path / "log" / "metrics_SyntheticDataLoader_run0.txt").exists()  # the baseline's files are still written


def test_cli_refit_serves_the_best_cell(tmp_path):
    path = G.CASES["small"]["path"]
    out = T.main(["--loader_name", "SyntheticDataLoader", "--path", path, "--neighborhood", "2",
                  "--base_log_path", str(tmp_path / "log"), "--svc_grid", "--svc_grid_c", "0:1:2",
                  "--svc_grid_gamma", "-8:-7:2", "--svc_grid_refit"], backend=EmuBackend())
    estimator = out[0][0]
    assert estimator is estimator.grid_search_.best_estimator_
    assert (estimator.C, estimator.gamma) == (estimator.grid_search_.best_params_["C"],
                                              estimator.grid_search_.best_params_["gamma"])


def test_hyperparamopt_still_refused_and_names_the_new_flag():
    with pytest.raises(NotImplementedError, match="--svc_grid"):
        T.main(["--hyperparamopt"], backend=EmuBackend())
    with pytest.raises(ValueError, match="lo:hi:n"):
        T.parse_decades("1,2", "--svc_grid_c")
