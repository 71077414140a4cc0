"""Hyper-parameter search for the kernel SVC on the device (reference classify/classic_ml_trainer.py:126-136:
`GridSearchCV(SVC(), {C, gamma}, cv=StratifiedShuffleSplit(2, test_size=0.1, random_state=42))`).

StratifiedShuffleSplit restates scikit-learn's splitter in numpy: its index stream is a deterministic function of the
labels and of numpy's legacy RandomState, pinned by tests/golden/reference_svm_grid.npz to scikit-learn 1.7.2's.

GridSearchSVC runs the whole C x gamma grid of a split as a handful of launches.  The inner products of a split depend
on neither parameter, so they are taken once (hypel_seg_gemm_f32, split-operand path); per chunk of gammas, sized from
free device memory, hypel_svm_kernel_planes_f32 turns them into one plane of K per gamma, hypel_svm_smo_grid solves every
(gamma, C, class pair) problem of the chunk in one launch -- one workgroup each, by the device function a single fit
runs --, and per gamma hypel_svm_scatter_coef_f32 + one product + hypel_svm_vote_score count the correct test rows of
its cells.  The host reads n_splits x n_cells integers (and the iteration counts).  As in svc.py there is no CPU
fallback; `backend` exists for the tests' numpy emulation of the same entry points."""
import warnings

import numpy as np
import torch

from hypelcnn_amd.backend import Ref, SVM_JOB_DTYPE, SVM_MAX_ITER_LIMIT, SVM_NOT_CONVERGED, SVM_RBF
from hypelcnn_amd.classic.svc import DEFAULT_MAX_ITER, NotConvergedError, SVC, _round_up, pair_table

# Issue order of the jobs of a smo_grid launch.  "c_desc": largest C first, within one C the longest pair first -- a
# large C lets the multipliers travel furthest, so those jobs are expected to run longest and should not start last.
# "plain": gamma-major table order.  tools/svm_grid_bench.py times both: on an MI355X "c_desc" is 8 % faster on the
# grss2013 fixture case and ties on the small one (NOTES.md, "SVC grid search"), so it is the default.
JOB_ORDERS = ("c_desc", "plain")
DEFAULT_JOB_ORDER = "c_desc"


class StratifiedShuffleSplit:
    """sklearn.model_selection.StratifiedShuffleSplit(n_splits, test_size=<float>, random_state=<int>): n_test =
    ceil(test_size n); per class floor + largest remainders (ties drawn from the generator), for the train part and then
    for the test part of what is left; one permutation per class; a final permutation of the train and of the test list."""

    def __init__(self, n_splits=10, test_size=None, train_size=None, random_state=None):
        if train_size is not None:
            raise NotImplementedError("StratifiedShuffleSplit(train_size=...): only a float test_size is restated")
        if isinstance(test_size, bool) or not isinstance(test_size, float) or not 0.0 < test_size < 1.0:
            raise NotImplementedError(f"StratifiedShuffleSplit(test_size={test_size!r}): a float in (0, 1); integer "
                                      f"sizes and the default are not restated")
        if isinstance(random_state, bool) or not isinstance(random_state, (int, np.integer)):
            raise NotImplementedError(f"StratifiedShuffleSplit(random_state={random_state!r}): an integer seed (the "
                                      f"split stream must be reproducible)")
        if int(n_splits) < 1:
            raise ValueError(f"StratifiedShuffleSplit(n_splits={n_splits})")
        self.n_splits, self.test_size, self.random_state = int(n_splits), test_size, int(random_state)

    def get_n_splits(self, X=None, y=None, groups=None):
        return self.n_splits

    @staticmethod
    def _approximate_mode(class_counts, n_draws, rng):
        continuous = class_counts / class_counts.sum() * n_draws
        floored = np.floor(continuous)
        need_to_add = int(n_draws - floored.sum())
        if need_to_add > 0:
            remainder = continuous - floored
            for value in np.sort(np.unique(remainder))[::-1]:
                (inds,) = np.where(remainder == value)
                add_now = min(len(inds), need_to_add)
                inds = rng.choice(inds, size=add_now, replace=False)
                floored[inds] += 1
                need_to_add -= add_now
                if need_to_add == 0:
                    break
        return floored.astype(int)

    def split(self, X, y, groups=None):
        y = np.asarray(y)
        if y.ndim != 1:
            raise NotImplementedError("StratifiedShuffleSplit.split: y is one label per row")
        n = len(y)
        n_test = int(np.ceil(self.test_size * n))
        n_train = n - n_test
        classes, y_indices = np.unique(y, return_inverse=True)
        n_classes = len(classes)
        class_counts = np.bincount(y_indices)
        if class_counts.min() < 2:
            raise ValueError("The least populated class in y has only 1 member, which is too few. The minimum number of "
                             "groups for any class cannot be less than 2.")
        if n_train < n_classes or n_test < n_classes:
            raise ValueError(f"train ({n_train}) and test ({n_test}) sizes must each reach the number of classes "
                             f"({n_classes})")
        class_indices = np.split(np.argsort(y_indices, kind="mergesort"), np.cumsum(class_counts)[:-1])
        rng = np.random.RandomState(self.random_state)
        for _ in range(self.n_splits):
            n_i = self._approximate_mode(class_counts, n_train, rng)
            t_i = self._approximate_mode(class_counts - n_i, n_test, rng)
            train, test = [], []
            for i in range(n_classes):
                perm = class_indices[i].take(rng.permutation(class_counts[i]), mode="clip")
                train.extend(perm[:n_i[i]])
                test.extend(perm[n_i[i]:n_i[i] + t_i[i]])
            yield rng.permutation(train), rng.permutation(test)


def parameter_grid(param_grid):
    """sklearn.model_selection.ParameterGrid's order: keys sorted, the last key fastest -- C outer, gamma inner."""
    return [{"C": float(c), "gamma": float(g)} for c in param_grid["C"] for g in param_grid["gamma"]]


def min_rank(mean):
    """rank_test_score: 'min' rank of the negated mean, NaN cells last (below the worst finite mean, as scikit-learn)."""
    mean = np.asarray(mean, np.float64)
    if np.isnan(mean).all():
        return np.ones(len(mean), np.int32)
    filled = np.where(np.isnan(mean), np.nanmin(mean) - 1.0, mean)
    return (1 + (filled[None, :] > filled[:, None]).sum(1)).astype(np.int32)


class GridSearchSVC:
    """GridSearchCV(SVC(), param_grid, cv=cv) for the RBF kernel SVC, every cell of a split solved and scored on the
    device.  Scores are accuracies on the split's test rows.  A cell with an unconverged pair scores NaN (scikit-learn's
    error_score=nan) and ranks last."""

    def __init__(self, param_grid, cv, tol=1e-3, max_iter=DEFAULT_MAX_ITER, refit=False, backend=None,
                 job_order=DEFAULT_JOB_ORDER, gamma_chunk=None):
        if sorted(param_grid) != ["C", "gamma"]:
            raise NotImplementedError(f"GridSearchSVC(param_grid keys {sorted(param_grid)}): the search is over 'C' and "
                                      f"'gamma' of SVC(kernel='rbf')")
        self.Cs = np.asarray(param_grid["C"], np.float64).reshape(-1)
        self.gammas = np.asarray(param_grid["gamma"], np.float64).reshape(-1)
        if len(self.Cs) == 0 or len(self.gammas) == 0 or not (self.Cs > 0).all() or not (self.gammas > 0).all():
            raise ValueError("GridSearchSVC: C and gamma are non-empty lists of positive floats")
        if not 0 < int(max_iter) <= SVM_MAX_ITER_LIMIT:
            raise ValueError(f"GridSearchSVC(max_iter={max_iter}): 1..{SVM_MAX_ITER_LIMIT} (the solver loop on the device "
                             f"is bounded)")
        if job_order not in JOB_ORDERS:
            raise ValueError(f"GridSearchSVC(job_order={job_order!r}): one of {JOB_ORDERS}")
        self.param_grid, self.cv, self.tol, self.max_iter, self.refit = param_grid, cv, float(tol), int(max_iter), refit
        self.job_order, self.gamma_chunk = job_order, gamma_chunk
        self._be = backend

    def _backend(self):
        if self._be is None:
            from hypelcnn_amd.backend import HipBackend
            self._be = HipBackend()
        return self._be

    def _gamma_chunk(self, per_gamma_bytes):
        if self.gamma_chunk:
            return max(1, min(int(self.gamma_chunk), len(self.gammas)))
        be = self._backend()
        free = 1 << 30
        if be.device.type == "cuda":
            free = torch.cuda.mem_get_info(be.device)[0]
        return max(1, min(len(self.gammas), int(free // 2 // max(1, per_gamma_bytes))))

    # ---- one split ---------------------------------------------------------------------------------------------
    def _split(self, X, yi, n_cls, train, test):
        """-> (n_correct [n_C, n_gamma], n_iter [n_gamma, n_C, n_pairs], unconverged pairs [n_C, n_gamma], n_test)"""
        be = self._backend()
        helper = SVC(kernel="rbf", gamma=1.0, backend=be)  # its row upload and its product, nothing else
        order = train[np.argsort(yi[train], kind="stable")]
        count = np.bincount(yi[order], minlength=n_cls).astype(np.int64)
        if count.min() == 0:
            raise ValueError("GridSearchSVC: a split's train part misses a class")
        start = np.concatenate([[0], np.cumsum(count)[:-1]])
        tab, total = pair_table(start, count)
        n_pairs, l_max = len(tab), int((tab["na"] + tab["nb"]).max())
        npp = max(32, _round_up(n_pairs, 4))
        n_c, n_g = len(self.Cs), len(self.gammas)
        xs, l, f, ldf = helper._rows(X, torch.from_numpy(order))
        xt, n_test, _, _ = helper._rows(X, torch.from_numpy(np.asarray(test)))
        mean = xs.view(l, ldf).double().mean(0).float().contiguous()  # (torch plumbing, once per split, as SVC.fit)
        tnorms = be.empty(n_test, torch.float64)
        be.call("svm_center_norms_f32", Ref(xs), ldf, l, f, Ref(mean), None)
        be.call("svm_center_norms_f32", Ref(xt), ldf, n_test, f, Ref(mean), Ref(tnorms))
        ldk = _round_up(l, 4)
        G, Gt = be.empty(l * ldk), be.empty(n_test * ldk)
        keep = helper._product(xs, ldf, l, xs, ldf, 1, f, G, ldk, l)
        keep += helper._product(xt, ldf, n_test, xs, ldf, 1, f, Gt, ldk, l)
        # The squared norm of a training row is the diagonal of G AS STORED (fp32), not the fp64 sum: the distance of a
        # row to itself is then exactly 0 and K's diagonal exactly 1 for every gamma.  With the fp64 norm the diagonal
        # is exp(-gamma e), e the fp32 rounding of the product (about 1 for these scenes): harmless at the reference's
        # gamma = 1e-9, but the grid goes up to 1e3, where it turns K = I into K = 0.9 I or worse and moves rho.  Off
        # the diagonal the change is half an fp32 ulp of |x|^2, what the product's own rounding already is.
        # (a strided copy of l values: torch plumbing, once per split, like the mean)
        norms = G.view(l, ldk).diagonal().double().contiguous()
        use_ws = 3 * l_max * 8 > 48 * 1024
        n_cols = n_c * npp
        per_gamma = 4 * ldk * (l + n_test) + 8 * n_c * total * (4 if use_ws else 1) + 64 * n_c * n_pairs
        chunk = self._gamma_chunk(per_gamma)
        plane, tplane = l * ldk, n_test * ldk
        K, Kt = be.empty(chunk * plane), be.empty(chunk * tplane)
        coef, bias, dec = be.empty(l * n_cols), be.empty(n_cols), be.empty(n_test * n_cols)
        tab_d = be.upload(tab)
        truth = be.upload(yi[np.asarray(test)].astype(np.int32))
        correct = be.zeros(n_g * n_c, torch.int32)  # gamma-major
        n_iter_all = np.zeros((n_g, n_c, n_pairs), np.int32)
        status_all = np.zeros((n_g, n_c, n_pairs), np.int32)
        for g0 in range(0, n_g, chunk):
            g1 = min(n_g, g0 + chunk)
            ng = g1 - g0
            n_jobs = ng * n_c * n_pairs
            gam = be.upload(self.gammas[g0:g1])
            be.call("svm_kernel_planes_f32", Ref(G), ldk, l, l, SVM_RBF, Ref(gam), ng, Ref(norms), Ref(norms), Ref(K),
                    plane)
            be.call("svm_kernel_planes_f32", Ref(Gt), ldk, n_test, l, SVM_RBF, Ref(gam), ng, Ref(tnorms), Ref(norms),
                    Ref(Kt), tplane)
            jobs = np.zeros((ng, n_c, n_pairs), SVM_JOB_DTYPE)
            for name in ("a0", "na", "b0", "nb"):
                jobs[name] = tab[name][None, None, :]
            cell = np.arange(ng)[:, None, None] * n_c + np.arange(n_c)[None, :, None]
            jobs["out_off"] = cell * total + tab["out_off"][None, None, :]
            jobs["k_off"] = np.arange(ng, dtype=np.int64)[:, None, None] * plane
            jobs["c"] = self.Cs[None, :, None]
            jobs = jobs.reshape(-1)
            order_d = None
            if self.job_order == "c_desc":
                issue = np.lexsort((-(jobs["na"] + jobs["nb"]), -jobs["c"])).astype(np.int32)
                order_d = be.upload(issue)
            jobs_d = be.upload(jobs)
            alpha_y = be.zeros(ng * n_c * total, torch.float64)
            rho, obj = be.zeros(n_jobs, torch.float64), be.zeros(n_jobs, torch.float64)
            n_iter, status = be.zeros(n_jobs, torch.int32), be.zeros(n_jobs, torch.int32)
            ws = be.zeros(3 * ng * n_c * total, torch.float64) if use_ws else None
            be.call("svm_smo_grid", Ref(K), ldk, Ref(jobs_d), None if order_d is None else Ref(order_d), n_jobs, l_max,
                    self.tol, self.max_iter, Ref(alpha_y), Ref(rho), Ref(obj), Ref(n_iter), Ref(status),
                    None if ws is None else Ref(ws))
            for gi in range(ng):
                be.call("svm_scatter_coef_f32", Ref(alpha_y, gi * n_c * total), Ref(rho, gi * n_c * n_pairs), Ref(tab_d),
                        n_pairs, n_c, total, l, npp, Ref(coef), n_cols, Ref(bias))
                keep += helper._product(Kt[gi * tplane:], ldk, n_test, coef, n_cols, 0, l, dec, n_cols, n_cols, bias)
                be.call("svm_vote_score", Ref(dec), n_cols, n_test, n_cls, n_c, npp, Ref(truth),
                        Ref(correct, (g0 + gi) * n_c))
            be.synchronize()  # the chunk's buffers and the products' tables die here
            keep.clear()
            n_iter_all[g0:g1] = n_iter.cpu().numpy().reshape(ng, n_c, n_pairs)
            status_all[g0:g1] = status.cpu().numpy().reshape(ng, n_c, n_pairs)
        n_correct = correct.cpu().numpy().reshape(n_g, n_c).T.copy()
        return n_correct, n_iter_all, (status_all == SVM_NOT_CONVERGED).sum(2).T.copy(), n_test

    # ---- the search --------------------------------------------------------------------------------------------
    def fit(self, X, y):
        y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
        classes, yi = np.unique(y, return_inverse=True)
        n_cls = len(classes)
        if n_cls < 2:
            raise ValueError("GridSearchSVC.fit: the number of classes has to be greater than one")
        if n_cls > 255:
            raise ValueError(f"GridSearchSVC.fit: {n_cls} classes; at most 255 (as SVC.fit)")
        if X.shape[0] != len(y):
            raise ValueError(f"GridSearchSVC.fit: {X.shape[0]} rows, {len(y)} labels")
        n_c, n_g = len(self.Cs), len(self.gammas)
        params = parameter_grid({"C": self.Cs, "gamma": self.gammas})
        res = {"params": params, "param_C": np.array([p["C"] for p in params]),
               "param_gamma": np.array([p["gamma"] for p in params])}
        scores, iters = [], []
        for s, (train, test) in enumerate(self.cv.split(X, y)):
            n_correct, n_iter, bad, n_test = self._split(X, yi, n_cls, np.asarray(train), np.asarray(test))
            iters.append(n_iter)
            it_max = n_iter.max(2).T
            score = n_correct.reshape(-1) / float(n_test)
            score[bad.reshape(-1) > 0] = np.nan
            res[f"split{s}_test_score"] = score
            res[f"split{s}_n_correct"] = n_correct.reshape(-1).astype(np.int64)
            res[f"split{s}_n_iter_max"] = it_max.reshape(-1).astype(np.int64)
            res[f"split{s}_not_converged"] = bad.reshape(-1).astype(np.int64)
            scores.append(score)
        self.n_splits_ = len(scores)
        self.n_iter_ = np.stack(iters)  # [split, gamma, C, pair]: what tools/svm_grid_bench.py's histogram reads
        mean = np.mean(np.stack(scores, 1), axis=1)
        res["mean_test_score"] = mean
        res["rank_test_score"] = min_rank(mean)
        self.cv_results_ = res
        n_nan = int(np.isnan(mean).sum())
        if n_nan == len(mean):
            raise NotConvergedError(f"GridSearchSVC.fit: every one of the {len(mean)} cells has a class pair that is not "
                                    f"converged after max_iter={self.max_iter} iterations; raise max_iter "
                                    f"(<= {SVM_MAX_ITER_LIMIT}) or tol")
        if n_nan:
            warnings.warn(f"GridSearchSVC.fit: {n_nan} of {len(mean)} cells have a class pair not converged after "
                          f"max_iter={self.max_iter} iterations; their score is NaN and they rank last", UserWarning)
        self.best_index_ = int(np.argmin(res["rank_test_score"]))
        self.best_params_ = dict(params[self.best_index_])
        self.best_score_ = float(mean[self.best_index_])
        if self.refit:
            self.best_estimator_ = SVC(kernel="rbf", gamma=self.best_params_["gamma"], C=self.best_params_["C"],
                                       tol=self.tol, max_iter=self.max_iter, backend=self._backend()).fit(X, y)
        return self
