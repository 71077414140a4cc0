"""Kernel support-vector classifier trained and served on the device (reference classify/classic_ml_trainer.py:46-54,
105: `sklearn.svm.SVC(...).fit(...)` / `.predict(...)`, i.e. libsvm's C-SVC with one-vs-one voting).

fit: the training rows are sorted by class (a class pair is then two contiguous row ranges), the whole kernel matrix K
is built once -- hypel_seg_gemm_f32 on the split-operand path, then hypel_svm_kernel_apply_f32 in place -- and
hypel_svm_smo_ovo solves all n (n - 1) / 2 pair problems in one launch, one workgroup per pair.  K is fp32 like
libsvm's Qfloat cache; the multipliers and the gradient are fp64 like libsvm's.  predict: per row chunk
K_block = kernel(rows, support vectors), decisions = K_block . coef - rho (the product again by hypel_seg_gemm_f32
against a dense [n_sv, n_pairs] coefficient matrix), labels by hypel_svm_vote.  A scene is never materialised as
rows x n_sv: the chunk is sized from free memory.

RBF rows are centred on the training mean before anything else (include/hypel.h, hypel_svm_center_norms_f32).
There is no CPU fallback and no second device: the `backend` argument exists so that the tests can run this file on
their numpy emulation of the same entry points."""
import numpy as np
import torch

from hypelcnn_amd import abi
from hypelcnn_amd.backend import (Ref, SVM_MAX_ITER_LIMIT, SVM_NOT_CONVERGED, SVM_PAIR_DTYPE, SVM_POLY, SVM_RBF)
from hypelcnn_amd.gemm_tables import GemmTables

GEMM_SPLIT6 = abi.const("HYPEL_GEMM_SPLIT6")
# Iteration cap of a pair (include/hypel.h: the solver loop is bounded).  libsvm's own max(10^7, 100 l) is too long for
# a shared device.  On the fixture problems of tests/golden/reference_classic_ml.json the emulation of this solver needs
# at most 1 120 iterations for a pair at tol = 1e-6 (recorded there per case as "emu_n_iter_max"; scikit-learn: 1 093);
# the cap is that times 100.
DEFAULT_MAX_ITER = 112000


class NotConvergedError(RuntimeError):
    pass


def _round_up(v, m):
    return (int(v) + m - 1) // m * m


def pair_list(n_classes):
    """libsvm's pair order: (0,1), (0,2) ... (0,n-1), (1,2) ..."""
    return [(a, b) for a in range(n_classes) for b in range(a + 1, n_classes)]


def pair_table(class_start, class_count):
    """hypel_svm_pair_t records of all pairs over rows sorted by class + the length of the alpha_y buffer."""
    pairs = pair_list(len(class_count))
    tab = np.zeros(len(pairs), SVM_PAIR_DTYPE)
    off = 0
    for p, (a, b) in enumerate(pairs):
        tab[p] = (class_start[a], class_count[a], class_start[b], class_count[b], off)
        off += int(class_count[a]) + int(class_count[b])
    return tab, off


def pack_model(alpha_y, tab, class_start, class_count):
    """Per-pair alpha * y -> libsvm's model layout.  Returns (sv, n_support, dual_coef [n_class - 1, n_sv], coef
    [n_sv, n_pairs]): sv = sorted positions (in class-sorted row order) of the vectors with a non-zero multiplier in ANY
    pair; a vector of class c holds its coefficient against class o in row o (o < c) or o - 1 (o > c)."""
    n_cls = len(class_count)
    l = int(np.sum(class_count))
    nonzero = np.zeros(l, bool)
    for rec in tab:
        a0, na, b0, nb, off = (int(rec[f]) for f in ("a0", "na", "b0", "nb", "out_off"))
        nonzero[a0:a0 + na] |= alpha_y[off:off + na] != 0
        nonzero[b0:b0 + nb] |= alpha_y[off + na:off + na + nb] != 0
    sv = np.flatnonzero(nonzero)
    pos = np.full(l, -1, np.int64)
    pos[sv] = np.arange(len(sv))
    n_support = np.array([int(nonzero[class_start[c]:class_start[c] + class_count[c]].sum()) for c in range(n_cls)],
                         np.int32)
    dual = np.zeros((n_cls - 1, len(sv)), np.float64)
    coef = np.zeros((len(sv), len(tab)), np.float64)
    for p, ((a, b), rec) in enumerate(zip(pair_list(n_cls), tab)):
        a0, na, b0, nb, off = (int(rec[f]) for f in ("a0", "na", "b0", "nb", "out_off"))
        for rows, vals, row_of_dual in ((np.arange(a0, a0 + na), alpha_y[off:off + na], b - 1),
                                        (np.arange(b0, b0 + nb), alpha_y[off + na:off + na + nb], a)):
            keep = nonzero[rows]
            dual[row_of_dual, pos[rows[keep]]] = vals[keep]
            coef[pos[rows[keep]], p] = vals[keep]
    return sv, n_support, dual, coef


class SVC:
    """The subset of sklearn.svm.SVC the reference uses, on the device.  decision_function is one-vs-one (pair order
    (0,1), (0,2) ...); with two classes it is the 1-D array scikit-learn returns (positive = classes_[1]) and
    dual_coef_ / intercept_ carry scikit-learn's sign flip for that case."""

    def __init__(self, kernel="rbf", gamma="scale", C=1.0, degree=3, coef0=0.0, tol=1e-3, max_iter=DEFAULT_MAX_ITER,
                 backend=None, chunk_rows=None):
        if kernel not in ("rbf", "poly"):
            raise NotImplementedError(f"SVC(kernel={kernel!r}): hypel_svm_kernel_apply_f32 evaluates 'rbf' and 'poly' "
                                      f"(the two the reference's classic_ml_trainer.py names)")
        if kernel == "poly" and not 1 <= int(degree) <= 3:
            raise NotImplementedError(f"SVC(kernel='poly', degree={degree}): the kernel evaluates degree 1..3")
        if not (isinstance(gamma, str) and gamma == "scale") and not (np.isscalar(gamma) and float(gamma) > 0):
            raise ValueError(f"SVC(gamma={gamma!r}): a positive float or 'scale'")
        if not 0 < int(max_iter) <= SVM_MAX_ITER_LIMIT:
            raise ValueError(f"SVC(max_iter={max_iter}): 1..{SVM_MAX_ITER_LIMIT} (the solver loop on the device is bounded)")
        self.kernel, self.gamma, self.C, self.degree, self.coef0 = kernel, gamma, float(C), int(degree), float(coef0)
        self.tol, self.max_iter, self.chunk_rows = float(tol), int(max_iter), chunk_rows
        self._be = backend

    def get_params(self):
        return {"C": self.C, "coef0": self.coef0, "degree": self.degree, "gamma": self.gamma, "kernel": self.kernel,
                "max_iter": self.max_iter, "tol": self.tol}

    # ---- plumbing ----------------------------------------------------------------------------------------------
    def _backend(self):
        if self._be is None:
            from hypelcnn_amd.backend import HipBackend
            self._be = HipBackend()
        return self._be

    def _rows(self, X, order=None):
        """[n, features] (numpy or tensor, any float dtype) -> flat fp32 device tensor [n, ldf], pad columns zero."""
        be = self._backend()
        t = torch.from_numpy(np.ascontiguousarray(X)) if isinstance(X, np.ndarray) else X
        if t.dim() != 2:
            raise ValueError(f"SVC: X must be [rows, features], got {tuple(t.shape)}")
        t = t.to(be.device)
        if order is not None:
            t = t.index_select(0, order.to(be.device))
        n, f = t.shape
        ldf = _round_up(f, 4)
        out = be.zeros(n * ldf) if ldf != f else be.empty(n * ldf)
        out.view(n, ldf)[:, :f] = t
        return out, n, f, ldf

    def _product(self, a, lda, rows, b, ldb, trans_b, k, c, ldc, n, bias=None):
        """c[rows, n] = a[rows, k] . op(b) (+ bias): one group, one segment."""
        be = self._backend()
        tables = GemmTables()
        tables.add_group(0, [(0, 0, int(k))], int(rows))
        garr, sarr, tarr, _ = tables.finalize(int(n))
        keep = [be.upload(garr), be.upload(sarr), be.upload(tarr)]
        be.call("seg_gemm_f32", Ref(a), int(lda), 0, Ref(b), int(ldb), int(trans_b), Ref(c), int(ldc), int(n),
                Ref(keep[0]), Ref(keep[1]), Ref(keep[2]), int(len(tarr)), None if bias is None else Ref(bias),
                GEMM_SPLIT6 if n > 16 else 0)
        return keep  # (the tables must outlive the launch)

    def _kernel_block(self, x, n, z, nz, znorm, out, ldo):
        """out[n, nz] = kernel(x rows, z rows); x is centred here (RBF)."""
        be = self._backend()
        rbf = self.kernel == "rbf"
        xnorm = None
        if rbf:
            xnorm = be.empty(n, torch.float64)
            be.call("svm_center_norms_f32", Ref(x), self._ldf, n, self._f, Ref(self._mean), Ref(xnorm))
        keep = self._product(x, self._ldf, n, z, self._ldf, 1, self._f, out, ldo, nz)
        be.call("svm_kernel_apply_f32", Ref(out), ldo, n, nz, SVM_RBF if rbf else SVM_POLY, self._gamma, self.coef0,
                self.degree, None if xnorm is None else Ref(xnorm), None if znorm is None else Ref(znorm))
        return keep

    # ---- fit ---------------------------------------------------------------------------------------------------
    def fit(self, X, y):
        be = self._backend()
        y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
        self.classes_, yi = np.unique(y, return_inverse=True)
        n_cls = len(self.classes_)
        if n_cls < 2:
            raise ValueError("SVC.fit: the number of classes has to be greater than one")
        if n_cls > 255:
            raise ValueError(f"SVC.fit: {n_cls} classes; hypel_svm_vote writes uint8 labels (the scene raster "
                             f"of --fullscene is uint8), so at most 255 classes")
        order = np.argsort(yi, kind="stable")
        class_count = np.bincount(yi, minlength=n_cls).astype(np.int64)
        class_start = np.concatenate([[0], np.cumsum(class_count)[:-1]])
        if self.gamma == "scale":
            var = float(X.var()) if isinstance(X, np.ndarray) else float(X.double().var(unbiased=False))
            self._gamma = 1.0 / (X.shape[1] * var) if var > 0 else 1.0
        else:
            self._gamma = float(self.gamma)
        xs, l, f, ldf = self._rows(X, torch.from_numpy(order))
        if l != len(y):
            raise ValueError(f"SVC.fit: {l} rows, {len(y)} labels")
        self._f, self._ldf = f, ldf
        rbf = self.kernel == "rbf"
        self._mean = None
        norms = None
        if rbf:
            # (column means of the rows just uploaded: torch plumbing, once per fit)
            self._mean = xs.view(l, ldf).double().mean(0).float().contiguous()
            norms = be.empty(l, torch.float64)
        if rbf:  # centred once, here; _kernel_block centres the rows a prediction brings
            be.call("svm_center_norms_f32", Ref(xs), ldf, l, f, Ref(self._mean), Ref(norms))
        ldk = _round_up(l, 4)
        K = be.empty(l * ldk)
        keep = self._product(xs, ldf, l, xs, ldf, 1, f, K, ldk, l)
        be.call("svm_kernel_apply_f32", Ref(K), ldk, l, l, SVM_RBF if rbf else SVM_POLY, self._gamma, self.coef0,
                self.degree, None if norms is None else Ref(norms), None if norms is None else Ref(norms))
        tab, total = pair_table(class_start, class_count)
        l_max = int((tab["na"] + tab["nb"]).max())
        n_pairs = len(tab)
        tab_d = be.upload(tab)
        alpha_y = be.zeros(total, torch.float64)
        rho, obj = be.zeros(n_pairs, torch.float64), be.zeros(n_pairs, torch.float64)
        n_iter, status = be.zeros(n_pairs, torch.int32), be.zeros(n_pairs, torch.int32)
        ws = be.zeros(3 * total, torch.float64) if 3 * l_max * 8 > 48 * 1024 else None
        be.call("svm_smo_ovo", Ref(K), ldk, Ref(tab_d), n_pairs, l_max, self.C, self.tol, self.max_iter, Ref(alpha_y),
                Ref(rho), Ref(obj), Ref(n_iter), Ref(status), None if ws is None else Ref(ws))
        be.synchronize()
        del keep
        self.n_iter_ = n_iter.cpu().numpy().copy()
        st = status.cpu().numpy()
        if (st == SVM_NOT_CONVERGED).any():
            bad = np.flatnonzero(st == SVM_NOT_CONVERGED)
            raise NotConvergedError(f"SVC.fit: {len(bad)} of {n_pairs} class pairs not converged after max_iter="
                                    f"{self.max_iter} iterations (first: pair {pair_list(n_cls)[bad[0]]}); raise max_iter "
                                    f"(<= {SVM_MAX_ITER_LIMIT}) or tol")
        ay = alpha_y.cpu().numpy()
        self._rho = rho.cpu().numpy().copy()
        self.pair_objective_ = obj.cpu().numpy().copy()
        self._pair_alpha_y, self._pair_table = ay, tab
        sv, self.n_support_, dual, coef = pack_model(ay, tab, class_start, class_count)
        if len(sv) == 0:
            raise NotConvergedError("SVC.fit: no support vectors")
        self.support_ = order[sv].astype(np.int32)
        flip = -1.0 if n_cls == 2 else 1.0  # scikit-learn's BaseLibSVM.fit flips both for the binary case
        self.dual_coef_ = flip * dual
        self.intercept_ = flip * -self._rho
        # device side of the model: support vectors (centred rows for RBF), their norms, dense coefficients, -rho
        idx = torch.from_numpy(sv).to(be.device)
        self._n_sv = len(sv)
        self._sv = xs.view(l, ldf).index_select(0, idx).contiguous().view(-1)
        self._sv_norm = norms.index_select(0, idx).contiguous() if rbf else None
        self._npp = max(32, _round_up(n_pairs, 4))  # the product's split-operand path wants n > 16
        w = np.zeros((self._n_sv, self._npp), np.float32)
        w[:, :n_pairs] = coef
        self._coef = be.upload(w)
        b = np.zeros(self._npp, np.float32)
        b[:n_pairs] = -self._rho
        self._bias = be.upload(b)
        self._labels_u8 = None
        if self.classes_.dtype.kind in "iu" and self.classes_.min() >= 0 and self.classes_.max() <= 255:
            self._labels_u8 = be.upload(self.classes_.astype(np.uint8))
        self._n_pairs = n_pairs
        return self

    # ---- predict -----------------------------------------------------------------------------------------------
    def _chunk(self, n):
        if self.chunk_rows:
            return max(1, min(int(self.chunk_rows), n))
        be = self._backend()
        per_row = 4 * (self._ldf + _round_up(self._n_sv, 4) + self._npp) + 16
        free = 1 << 30
        if be.device.type == "cuda":
            free = torch.cuda.mem_get_info(be.device)[0]
        return max(1, min(n, int(free // 4 // per_row), 1 << 18))

    def _decide(self, x, n, dec, labels=None, points=None, raster=None, raster_w=0):
        """x: flat [n, ldf] fp32 device rows (overwritten by their centred form) -> dec [n, npp]; labels into `labels`
        (in order) or into `raster` at `points`."""
        be = self._backend()
        ldg = _round_up(self._n_sv, 4)
        g = be.empty(n * ldg)
        keep = self._kernel_block(x, n, self._sv, self._n_sv, self._sv_norm, g, ldg)
        keep += self._product(g, ldg, n, self._coef, self._npp, 0, self._n_sv, dec, self._npp, self._npp, self._bias)
        n_cls = len(self.classes_)
        if raster is not None:
            be.call("svm_vote", Ref(dec), self._npp, n, n_cls, Ref(self._labels_u8), Ref(points), Ref(raster),
                    int(raster_w))
        elif labels is not None:
            be.call("svm_vote", Ref(dec), self._npp, n, n_cls, None, None, Ref(labels), 0)
        be.synchronize()  # g and the tables die here
        del keep

    def _run(self, X, want_dec):
        be = self._backend()
        if not hasattr(self, "support_"):
            raise RuntimeError("SVC: fit first")
        n = X.shape[0]
        if X.shape[1] != self._f:
            raise ValueError(f"SVC: X has {X.shape[1]} features, the model was fitted on {self._f}")
        idx = be.zeros(n, torch.uint8)
        decs = np.zeros((n, self._n_pairs), np.float32) if want_dec else None
        step = self._chunk(n)
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            x, m, _, _ = self._rows(X[r0:r1])
            dec = be.empty(m * self._npp)
            self._decide(x, m, dec, labels=idx[r0:r1])
            if want_dec:
                decs[r0:r1] = dec.view(m, self._npp)[:, :self._n_pairs].cpu().numpy()
        return idx.cpu().numpy(), decs

    def predict(self, X):
        idx, _ = self._run(X, False)
        return self.classes_[idx]

    def decision_function(self, X):
        _, dec = self._run(X, True)
        return -dec.reshape(-1) if len(self.classes_) == 2 else dec

    def predict_scene(self, arrays, raster, raster_w):
        """Whole-scene path: `arrays` is a common_nn_ops.SceneArrays fed with the padded scene and the (x, y) targets,
        `raster` a flat uint8 device tensor that receives classes_[winner] at y * raster_w + x.  Patches are cut on the device (hypel_gather_patches_f32) chunk by chunk."""
        be = self._backend()
        if self._labels_u8 is None:
            raise ValueError("SVC.predict_scene: class labels must be integers in 0..255 for the uint8 raster")
        n = len(arrays)
        step = self._chunk(n)
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            patches, pts = arrays.gather(torch.arange(r0, r1, device=be.device))
            x, m, _, _ = self._rows(patches.reshape(r1 - r0, -1))
            dec = be.empty(m * self._npp)
            self._decide(x, m, dec, points=pts.reshape(-1), raster=raster, raster_w=raster_w)
