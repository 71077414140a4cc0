"""-m gpu: the classifier's layout, LRN, loss-head, metric, gather and copy kernels (csrc/elementwise.hip, csrc/data.hip)
through the C-ABI, each against a plain definition of the same operation: float64 NumPy with bounds derived as counts of
fp32 roundings, or -- pure data movement -- a NumPy / torch composition, bit for bit (tests/head_kernel_cases.py holds
the case tables, the operand layouts, the references and the derivations; tests/test_head_kernel_cases_emu.py runs the
same cases through the executable spec on the CPU and asserts that a plain float32 evaluation meets every bound).

Every operand is a window of a sentinel-filled allocation, at a 16-byte base and at one that is only 4-byte aligned, and
everything outside an output's window must keep the sentinel's bits.  No case is skipped or left out of a comparison.
Every tolerance is bit exactness, a bound derived in a docstring of tests/head_kernel_cases.py, or one of the measured
powf figures below times the stated margin."""
import pytest

from tests import head_kernel_cases as H
from tests import parity_util as PU
from tests.test_gpu_step_tail import LIBM_MARGIN

pytestmark = pytest.mark.gpu

# Accuracy of the device powf in the two calls of the LRN kernels, measured on an MI355X with
# tools/exp/probe/libm_ulp_probe.hip: 8192 arguments per range, spread evenly in log(s), against the host's double pow, in
# fp32 ulps of the result (subnormal spacing below FLT_MIN).  s = bias + alpha * (window sum of x^2) over what the cases
# produce: about the bias (operands of 1e-3), up to 1e11 (384 operands of 1e3), 1e25 .. 1e31 (one operand of 1e15).
#   beta = 0.5, bias 1     [1, 1.01]   [1, 1e11]   [1e25, 1e31]      beta = 0.75, bias 2   [2, 2.02]   [2, 1e11]   [1e25, 1e31]
#   powf(s, -0.5)           0.6343      1.1237      1.2415            powf(s, -0.75)         1.0650      1.1561      1.1961
#   powf(s, -1.5)           0.6181      1.1968      1.2180            powf(s, -1.75)         1.2439      1.1599      0.9987
# (powf(s, -1.5) on [1e25, 1e31] ends among the subnormals -- smallest result 3e-47, below the last of them;
# powf(s, -1.75) there underflows throughout.)  The largest figure of each call stands below; like EXPF_ULP_MEASURED they
# are multiplied by LIBM_MARGIN = 2: the device libm carries no written ulp contract and the grid is a sample.
POWF_ULP_MEASURED = {(0.5, "fwd"): 1.2415, (0.5, "bwd"): 1.2180, (0.75, "fwd"): 1.1961, (0.75, "bwd"): 1.2439}
POWF_ULP = {k: v * LIBM_MARGIN for k, v in POWF_ULP_MEASURED.items()}


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def report():
    rep = H.Report()
    yield rep
    print("\n" + "\n".join(rep.lines()))


# ------------------------------------------------------------------------------------------------------------ 1. layout
@pytest.mark.parametrize("c", H.LAYOUT_C)
def test_h1_layout_data_bits_pad_zeros_round_trip(hip, c):
    """head_kernel_cases.run_layout at every ld of {c, c + 1, c + 3, next multiple of 4} and p * n of {1, 3, 4, 5, 17}"""
    H.run_layout_c(PU.Both(hip), c)


def test_h1_layout_second_trip(hip):
    n, p, c = H.LAYOUT_BIG
    H.run_layout(PU.Both(hip), n, p, c, c + 3, 1)


# --------------------------------------------------------------------------------------------------------------- 2. LRN
@pytest.mark.parametrize("c", H.LRN_C)
def test_h2_lrn_forward_backward_accumulate(hip, report, c):
    """head_kernel_cases.run_lrn (bounds: lrn_bounds) at radius {0, 5, c}, rows {1, 3, 257}, both parameter sets, the
    rows cycling through the five operand regimes"""
    H.run_lrn_c(PU.Both(hip), report, c, POWF_ULP)


def test_h2_lrn_grid_stride(hip, report):
    rows, c, radius = H.LRN_BIG
    for k, params in enumerate(H.LRN_PARAMS):
        H.run_lrn(PU.Both(hip), report, rows, c, radius, params, k, POWF_ULP)


# ------------------------------------------------------------------------------------------------ 3. MSE, partials, sum
@pytest.mark.parametrize("shape", H.MSE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h3_mse_every_form_of_one_operand_set(hip, report, shape):
    """head_kernel_cases.run_mse (bounds: mse_bounds): flat4 and general dispatch, offsets, leading dimensions, no da"""
    H.run_mse(PU.Both(hip), report, *shape)


def test_h3_mse_flat4_second_trip(hip, report):
    H.run_mse(PU.Both(hip), report, *H.MSE_FLAT_BIG, forms=[H.MSE_FORMS[0], H.MSE_FORMS[7]])


@pytest.mark.parametrize("kind", ["one", "span"])
@pytest.mark.parametrize("shape", [(16, 16), (1, 257)], ids=["flat4", "general"])
def test_h3_mse_one_term_and_wide_span(hip, report, shape, kind):
    """a == b but for one element: the MSE is that term; |a - b| from 1e-20 to 1e15: the sum is its largest terms"""
    H.run_mse(PU.Both(hip), report, *shape, kind=kind, forms=[H.MSE_FORMS[0], H.MSE_FORMS[8]])


@pytest.mark.parametrize("count", H.SUM_COUNTS)
def test_h3_sum_mixed_signs(hip, report, count):
    import numpy as np
    rng = np.random.default_rng(count)
    H.run_sum(PU.Both(hip), report, (rng.standard_normal(count) * 10.0 ** rng.uniform(-2, 2, count)).astype(np.float32), f"n{count}")


def test_h3_sum_cancelling_pairs(hip, report):
    """+v, -v inside one thread's chain: exactly 0; across blocks: within the bound of sum |x|"""
    import numpy as np
    H.run_sum(PU.Both(hip), report, H.sum_pairs_in_chain(np.random.default_rng(1)), "pairs in chain", exact_zero=True)
    H.run_sum(PU.Both(hip), report, H.sum_pairs_across_blocks(np.random.default_rng(2)), "pairs across blocks")


# ------------------------------------------------------------------------------------------------------------ 4. argmax
@pytest.mark.parametrize("c", H.ARGMAX_C)
def test_h4_argmax_confusion_and_scatter(hip, c):
    """head_kernel_cases.run_argmax_confusion / run_argmax_scatter at n of {1, 127, 128, 129}, ld of {c, c + 3} with +inf
    in the pad: ties, -inf, +-0, one ulp, +inf and the NaN rule of include/hypel.h; ignored labels; NULL outputs"""
    H.run_argmax_c(PU.Both(hip), c)


def test_h4_confusion_one_cell(hip):
    H.run_confusion_one_cell(PU.Both(hip))


# --------------------------------------------------------------------------------------------- 5. gathers, augmentation
@pytest.mark.parametrize("cc,cl", H.GATHER_CC_CL)
def test_h5_gather_patches(hip, cc, cl):
    for p in (1, 3):
        for n in (1, 6):
            H.run_gather(PU.Both(hip), cc, cl, p, n)


def test_h5_gather_patches_block_walk(hip):
    n, p = H.GATHER_BIG
    H.run_gather(PU.Both(hip), 92, 3, p, n)


@pytest.mark.parametrize("nb", [0, 1, 2, 3])
def test_h5_gather_patches_2x(hip, nb):
    H.run_gather_2x(PU.Both(hip), nb, 5, 1)
    H.run_gather_2x(PU.Both(hip), nb, 94, 2)
    H.run_gather_2x(PU.Both(hip), nb, 190, 2, n=1)


@pytest.mark.parametrize("c", H.AUGMENT_C)
def test_h5_augment_patches(hip, c):
    H.run_augment_c(PU.Both(hip), c)


def test_h5_augment_refuses_ratio_with_alt(hip):
    msg = H.run_augment_refusal(hip)
    assert "hypel_augment_patches_f32" in msg and "shadow_ratio && shadow_alt" in msg
    assert "shadow_ratio && shadow_alt" in hip.lib.hypel_last_error().decode()


# -------------------------------------------------------------------------------------------- 6. chanmap_bwd, copies
@pytest.mark.parametrize("cin", H.CHANMAP_CIN)
@pytest.mark.parametrize("table", [True, False], ids=["table", "identity"])
def test_h6_chanmap_bwd(hip, report, cin, table):
    for rows in H.CHANMAP_ROWS:
        for layout in ("aligned", "odd"):
            for accumulate in (0, 1):
                H.run_chanmap(PU.Both(hip), report, cin, rows, layout, accumulate, table)


def test_h6_copy_blocks(hip):
    H.run_copy_blocks(PU.Both(hip))


def test_h6_copy_pair(hip):
    H.run_copy_pair(PU.Both(hip))
