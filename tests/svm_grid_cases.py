"""TEST INFRASTRUCTURE shared by tests/golden/make_reference_svm_grid.py and the grid-search tests: the fixture cases,
their inputs (re-made from SyntheticDataLoader as tests/svm_cases.py does, never stored), the label vectors that pin the
splitter, and the checks of a fitted GridSearchSVC against scikit-learn's stored GridSearchCV -- the same code on the
emulation and on the device.

Contract of a case (bounds measured on scikit-learn alone when the fixture is written, none from the code under test):
  counts     per split and cell |n_correct - fixture| <= the cell's unstable test rows; a row is unstable by
             svm_cases.unstable_mask with delta = 2 max |dec(tol 1e-3) - dec(tol 1e-6)| of scikit-learn on that cell
  cap        unstable (row, cell) entries are at most 3 % of a case's entries (asserted by the maker)
  best cell  all counts equal -> best_index_, best_params_, rank_test_score equal, best_score_ to 1e-12; otherwise the
             product's best cell has a fixture mean score within (its unstable rows over the splits) / (rows scored)
             of the fixture's best score."""
import json
import os

import numpy as np

from tests import svm_cases as S

JSON_PATH = os.path.join(S.GOLDEN, "reference_svm_grid.json")
NPZ_PATH = os.path.join(S.GOLDEN, "reference_svm_grid.npz")

N_SPLITS, TEST_SIZE, SEED, TOL = 2, 0.1, 42, 1e-3  # reference classic_ml_trainer.py:130; SVC()'s own tol
# decades lo:hi:n as --svc_grid_c / --svc_grid_gamma take them.  "grss2013": see the fixture JSON's "choice" for why the
# scene is the loader's grss2013 at half its height and width and the grid a 5 x 5 window of the reference's.
CASES = {
    "small": dict(path="grss2013:bands=8:classes=4:h=20:w=24", C=(-2, 10, 13), gamma=(-9, 3, 13)),
    "grss2013": dict(path="grss2013:h=30:w=40", C=(-2, 2, 5), gamma=(-9, -5, 5)),
}
# label vectors that pin the splitter alone: (labels, n_splits, test_size, seed)
SPLIT_CASES = {
    "remainder_ties": (np.repeat(np.arange(5), 13), 2, 0.1, 42),          # 5 equal classes: every remainder ties
    "class_of_two": (np.repeat(np.arange(4), [2, 30, 17, 11]), 2, 0.1, 42),
    "two_classes": (np.repeat([7, 3], [41, 26]), 2, 0.1, 42),              # unsorted label values
    "three_splits": (np.repeat(np.arange(6), [9, 9, 14, 20, 9, 33])[::-1].copy(), 3, 0.25, 7),
    "interleaved": (np.arange(120) % 7, 2, 0.1, 42),
}


def decades(spec):
    lo, hi, n = spec
    return np.logspace(lo, hi, n)


def grid_of(case):
    return {"C": decades(CASES[case]["C"]), "gamma": decades(CASES[case]["gamma"])}


_cache = {}


def load_case_data(case):
    """(X, y) flattened float32 training rows, as classic_ml_trainer reads them."""
    path = CASES[case]["path"]
    if path not in _cache:
        from hypelcnn_amd.importer.InMemoryImporter import InMemoryImporter
        tr = InMemoryImporter().read_data_set("SyntheticDataLoader", path, 0.1, 0, S.NEIGHBORHOOD, False)[0]
        _cache[path] = (tr.data.reshape(len(tr.data), -1), tr.labels)
    return _cache[path]


def load_fixture():
    with open(JSON_PATH) as f:
        meta = json.load(f)
    return meta, np.load(NPZ_PATH)


def unstable_counts(case, fx):
    """[n_splits, n_cells] number of unstable test rows"""
    shape = tuple(fx[f"{case}/unstable_shape"])
    bits = np.unpackbits(fx[f"{case}/unstable"])[:int(np.prod(shape))].reshape(shape).astype(bool)
    return bits.sum(2)


def check_splits(splitter_cls, labels, n_splits, test_size, seed, fx, key):
    got = list(splitter_cls(n_splits=n_splits, test_size=test_size, random_state=seed).split(np.zeros((len(labels), 1)),
                                                                                               labels))
    assert len(got) == n_splits
    for s, (train, test) in enumerate(got):
        assert np.array_equal(train, fx[f"{key}/train{s}"]), (key, s, "train")
        assert np.array_equal(test, fx[f"{key}/test{s}"]), (key, s, "test")


def check_search(search, case, meta, fx):
    """Tests 2 and 3 of the contract; prints every figure before it asserts."""
    m = meta["cases"][case]
    res = search.cv_results_
    ref_counts = fx[f"{case}/n_correct"]
    un = unstable_counts(case, fx)
    n_test = m["n_test"]
    got = np.stack([res[f"split{s}_n_correct"] for s in range(N_SPLITS)])
    diff = np.abs(got - ref_counts)
    bad = np.stack([res[f"split{s}_not_converged"] for s in range(N_SPLITS)])
    it_max = int(np.stack([res[f"split{s}_n_iter_max"] for s in range(N_SPLITS)]).max())
    print(f"{case}: cells {got.shape[1]}, counts differing {int((diff > 0).sum())}, beyond the unstable rows "
          f"{int((diff > un).sum())}, max |diff| {int(diff.max())}, unstable entries {int(un.sum())} of "
          f"{un.size * n_test}, unconverged cells {int((bad > 0).sum())}, iterations max {it_max}")
    assert m["constant_kernel_cells_rho_within_delta"] == 0  # no gamma >= 1 cell decides by the sign of a rounding
    assert (bad == 0).all()
    assert (diff <= un).all()
    assert [p["C"] for p in res["params"]] == fx[f"{case}/param_C"].tolist()
    assert [p["gamma"] for p in res["params"]] == fx[f"{case}/param_gamma"].tolist()
    ref_mean = fx[f"{case}/mean_test_score"]
    print(f"{case}: best {search.best_index_} {search.best_params_} score {search.best_score_:.6f}; fixture "
          f"{m['best_index']} {m['best_params']} score {m['best_score']:.6f}")
    if (diff == 0).all():
        assert search.best_index_ == m["best_index"] and search.best_params_ == m["best_params"]
        assert np.array_equal(res["rank_test_score"], fx[f"{case}/rank_test_score"])
        assert abs(search.best_score_ - m["best_score"]) <= 1e-12
        assert np.abs(res["mean_test_score"] - ref_mean).max() <= 1e-12
    else:
        slack = un[:, search.best_index_].sum() / float(N_SPLITS * n_test)
        assert m["best_score"] - ref_mean[search.best_index_] <= slack + 1e-12
    return it_max
