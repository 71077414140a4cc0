"""-m gpu: the loss tail of the shadow-GAN train op (csrc/gan.hip: nce_loss, l2norm_*, gan_loss, loss_terms_slots +
loss_finalize_slots) through the C-ABI against the float64 spec, at more than the one shape per kernel that
tests/test_gpu_kernels.py runs: the generic patch-NCE kernel, the l2norm clamp and its 16 384-element switch, c = 1 and
c > 256 loss terms, exact L1 ties, a regulariser longer than one grid pass.  Every row operand is a slice with its own
leading dimension inside a sentinel-filled allocation (tests/parity_util.Arena).  Cases: tests/gan_kernel_cases.py."""
import numpy as np
import pytest

from tests import gan_kernel_cases as C
from tests.parity_util import Both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


def _report(res, names):
    for nm in names:
        h, e = res[nm]
        print(nm, "max |device - spec| / max(1, max|spec|) =", np.abs(h - e).max() / max(1.0, np.abs(e).max()))


# ------------------------------------------------------------------------------------------------------------ patch-NCE
@pytest.mark.parametrize("n", C.NCE_N)
@pytest.mark.parametrize("pe", C.NCE_PE, ids=lambda pe: f"P{pe[0]}E{pe[1]}")
def test_nce_loss_shapes_strides_and_flags(hip, pe, n):
    """(6, 2), (7, 2): the compile-time kernels; (5, 3), (1, 4), (8, 2): the generic kernel.  ldg / ldr / lddg / lddr
    pairwise different with offsets; dg only, dr only, neither; both accumulate flags on pre-filled gradients and on the
    loss; sentinels around every window (inside run_nce)."""
    C.close_all(C.run_nce(Both(hip), *pe, n), C.NCE_TOL, f"nce P={pe[0]} E={pe[1]} n={n}:")


@pytest.mark.parametrize("pe", C.NCE_BIG, ids=lambda pe: f"P{pe[0]}E{pe[1]}")
def test_nce_loss_large_logits(hip, pe):
    """Embeddings scaled so that the largest |logit / tau| is 200: the exponentials span e^-400 .. 1 once the maximum is
    taken out.  A regime no existing test has, so the tolerance is measured: a float32 NumPy evaluation of the same
    formula lies within 2.04e-6 ((7, 2)) / 1.0e-6 ((5, 3)) of max(1, max|spec|) of the float64 spec, largest over the
    loss, dg and dr of every step (gan_kernel_cases.NCE_BIG_F32_ERR); the device is allowed 4 x that."""
    res = C.run_nce(Both(hip), *pe, C.NCE_BIG_N, big=True)
    _report(res, sorted(res))
    tol = C.measured_tol(C.NCE_BIG_F32_ERR[pe])
    C.close_all(res, {"loss": tol, "dg": tol, "dr": tol}, f"nce P={pe[0]} E={pe[1]} large logits:")
    for pair in res.values():
        assert np.isfinite(pair[0]).all()


@pytest.mark.parametrize("pe", [(6, 2), (5, 3)], ids=lambda pe: f"P{pe[0]}E{pe[1]}")
def test_nce_loss_all_equal_logits(hip, pe):
    """g = 0: every logit is 0, the loss is P * log(P^2) per sample (weight 10: the first step overwrites nothing but
    accumulates onto 3)."""
    p = pe[0]
    res = C.run_nce(Both(hip), *pe, 65, zero_g=True)
    want = 10.0 * p * np.log(p * p)
    np.testing.assert_allclose(res["loss2"][0][0], want, rtol=1e-5)  # step 2 overwrites the loss
    np.testing.assert_allclose(res["loss0"][0][0], 3.0 + want, rtol=1e-5)
    C.close_all(res, C.NCE_TOL)


# --------------------------------------------------------------------------------------------------------------- l2norm
@pytest.mark.parametrize("case", C.L2N_CASES, ids=C.case_id)
def test_l2norm_clamp_switch_and_strides(hip, case):
    """l2norm_fwd / _bwd, _parts (3 parts), _segs (3 parts x 2 segments) at 37, 8192 (x 2 = 16 384 elements: the last
    size of the register kernel) and 8193 rows (the looping kernel); four different lds with offsets, both accumulate
    flags, sentinels.  special: an all-zero part (y = 0, stat = [0, 1e6], dx = dy * 1e6) and a part whose sum x^2 lies
    just above the clamp of 1e-12.

    Near the clamp the outputs are far from 1 (stat[0] ~ 1e-12, stat[1] ~ 1e6), so the bound is relative to max|spec|
    of each output and measured: a float32 NumPy evaluation lies within 1.45e-7 of the float64 spec (largest over y,
    stat, dx and all cases, gan_kernel_cases.L2N_TINY_F32_ERR); the device is allowed 4 x that."""
    C.check_l2norm(Both(hip), *case)


# ------------------------------------------------------------------------------------------------------- tfgan losses
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("rows,c", C.LOSS_SHAPES)
def test_gan_loss_shapes_strides_and_flags(hip, rows, c, mode):
    """c = 1, 37, 300 (> 256: a thread walks two columns) x rows = 1, 300, 3000; a third of the L1 elements with a == b
    (gradient 0); distinct lda / ldb / ldda / lddb; da or db absent; both accumulate flags; the loss over three
    accumulating rounds onto 3."""
    C.close_all(C.run_gan_loss(Both(hip), mode, rows, c), C.GAN_LOSS_TOL, f"gan_loss mode={mode} {rows}x{c}:")


@pytest.mark.parametrize("rows,c", C.LOSS_SHAPES)
def test_loss_terms_slots_shapes_strides_and_flags(hip, rows, c):
    """The same through hypel_loss_terms_slots + hypel_loss_finalize_slots: modes 0-3 in one launch over one arena."""
    C.close_all(C.run_loss_slots(Both(hip), rows, c), C.SLOTS_TOL, f"loss slots {rows}x{c}:")


def test_loss_terms_slots_long_regulariser(hip):
    """Mode 3 over 300 001 weights: more than one pass of 1024 blocks x 256 threads.  A sum of that length is a new
    regime: a float32 NumPy evaluation of 3 + 3 * 0.5e-3 * sum w^2 lies within 1.32e-7 of the float64 spec (relative to
    the loss; dw: identical), gan_kernel_cases.L2_LONG_F32_ERR; the device is allowed 4 x that, and never less than one
    ulp of the float32 result."""
    res = C.run_loss_slots(Both(hip), 1, 1, nw=C.L2_LONG, only_l2=True)
    _report(res, ["loss", "dw"])
    for nm in ("loss", "dw"):
        C.close_all({nm: res[nm]}, {nm: C.measured_tol(C.L2_LONG_F32_ERR[nm])}, "long regulariser:")
