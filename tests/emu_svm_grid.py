"""TEST INFRASTRUCTURE: numpy twins of the grid-search entry points (include/hypel.h, ABI 8: hypel_svm_kernel_planes_f32,
hypel_svm_smo_grid, hypel_svm_scatter_coef_f32, hypel_svm_vote_score), attached to tests/emu_backend.EmuBackend on
import, next to tests/emu_svm.py whose kernel_values, smo_pair and vote they reuse."""
import numpy as np

from hypelcnn_amd.backend import SVM_JOB_DTYPE, SVM_MAX_ITER_LIMIT, SVM_PAIR_DTYPE
from tests.emu_backend import EmuBackend, _arr, _mat
from tests.emu_svm import RBF, kernel_values, smo_pair, vote


def job_rows(rec):
    a0, na, b0, nb = (int(rec[f]) for f in ("a0", "na", "b0", "nb"))
    return np.concatenate([np.arange(a0, a0 + na), np.arange(b0, b0 + nb)]), na, nb


def _k_svm_kernel_planes_f32(self, g, ld, rows, cols, kind, gammas, n_gamma, row_norms, col_norms, out, plane_stride):
    assert kind == RBF, "rbf only"
    assert plane_stride >= rows * ld
    g_at, o_at = g.ptr(), out.ptr()
    assert o_at + 4 * ((n_gamma - 1) * plane_stride + rows * ld) <= g_at or g_at + 4 * rows * ld <= o_at, "out of place"
    m = _mat(g, ld, rows, cols)
    before = m.copy()
    rn, cn = _arr(row_norms, np.float64)[:rows], _arr(col_norms, np.float64)[:cols]
    gam = _arr(gammas, np.float64)[:n_gamma]
    o = _arr(out)
    # a plane is what hypel_svm_kernel_apply_f32 leaves in place: where rows are walked in groups of four columns (ld and
    # plane_stride multiples of 4) the pad columns of a row's last group hold g's own values, any further one is not written
    last = (cols + 3) // 4 * 4 if ld % 4 == 0 and plane_stride % 4 == 0 else cols
    pads = _mat(g, ld, rows, last)[:, cols:].copy()
    for p in range(n_gamma):
        plane = np.lib.stride_tricks.as_strided(o[p * plane_stride:], (rows, last), (ld * 4, 4))
        plane[:, :cols] = kernel_values(before, RBF, float(gam[p]), 0.0, 0, rn, cn).astype(np.float32)
        plane[:, cols:] = pads
    assert np.array_equal(m, before), "out of place: g is left intact"


def _k_svm_smo_grid(self, k, ldk, jobs, order, n_jobs, l_max, tol, max_iter, alpha_y, rho, obj, n_iter, status, ws):
    assert 0 < max_iter <= SVM_MAX_ITER_LIMIT, "the iteration cap is bounded"
    tab = jobs.t.numpy()[jobs.off:jobs.off + n_jobs * SVM_JOB_DTYPE.itemsize].view(SVM_JOB_DTYPE)
    issue = np.arange(n_jobs) if order is None else _arr(order, np.int32)[:n_jobs]
    assert sorted(issue.tolist()) == list(range(n_jobs)), "order is a permutation of the jobs"
    kf = _arr(k)
    for j in issue:  # (any order gives the same result: the jobs are independent)
        rec = tab[j]
        rows, na, nb = job_rows(rec)
        assert na + nb <= l_max and (3 * l_max * 8 <= 48 * 1024 or ws is not None)
        sub = kf[int(rec["k_off"]) + rows[:, None] * ldk + rows[None, :]]
        ay, r, o, it, st = smo_pair(sub, na, float(rec["c"]), tol, max_iter)
        off = int(rec["out_off"])
        _arr(alpha_y, np.float64)[off:off + na + nb] = ay
        _arr(rho, np.float64)[j] = r
        _arr(obj, np.float64)[j] = o
        _arr(n_iter, np.int32)[j] = it
        _arr(status, np.int32)[j] = st


def _k_svm_scatter_coef_f32(self, alpha_y, rho, pairs, n_pairs, n_c, cell_stride, l, npp, coef, ldc, bias):
    assert npp >= n_pairs and ldc >= n_c * npp
    tab = pairs.t.numpy()[pairs.off:].view(SVM_PAIR_DTYPE)[:n_pairs]
    ay = _arr(alpha_y, np.float64)
    w = _mat(coef, ldc, l, n_c * npp)
    w[...] = 0.0
    b = _arr(bias)[:n_c * npp]
    b[...] = 0.0
    for ci in range(n_c):
        for p, rec in enumerate(tab):
            rows, na, nb = job_rows(rec)
            off = ci * cell_stride + int(rec["out_off"])
            w[rows, ci * npp + p] = ay[off:off + na + nb].astype(np.float32)
            b[ci * npp + p] = np.float32(-_arr(rho, np.float64)[ci * n_pairs + p])


def _k_svm_vote_score(self, dec, ld, rows, n_classes, n_cells, npp, truth, correct):
    n_pairs = n_classes * (n_classes - 1) // 2
    assert 2 <= n_classes <= 255 and npp >= n_pairs and ld >= n_cells * npp
    d = _mat(dec, ld, rows, n_cells * npp)
    t = _arr(truth, np.int32)[:rows]
    c = _arr(correct, np.int32)
    for cell in range(n_cells):
        c[cell] += int((vote(d[:, cell * npp:cell * npp + n_pairs], n_classes) == t).sum())


for _name, _fn in list(globals().items()):
    if _name.startswith("_k_svm_"):
        setattr(EmuBackend, _name[1:], _fn)
