"""Every case of tests/gan_kernel_cases.py through the executable spec alone (no GPU): the strided launch equals the
contiguous one exactly, the sentinels around every window hold, no knife-edge row is left after 20 rounds (asserted where
the cases are drawn), outputs are finite except in the NaN case -- so that what tests/test_gpu_gan_stacks.py and
tests/test_gpu_gan_losses.py later hold the kernels to is a consistent statement.  Then the comparison helpers themselves:
each must refuse a copy of the spec output with one planted defect.  The measured tolerances of the new regimes are
re-measured and held to the constants the GPU tests use."""
import numpy as np
import pytest

from tests import gan_kernel_cases as C
from tests.parity_util import SENT, Arena, SpecOnly, arena, assert_close, assert_same_bits


# ------------------------------------------------------------------------------------------- spec-only run of the tables
@pytest.mark.parametrize("case", C.GEN_STRIDED, ids=C.case_id)
def test_generator_strided_cases(case):
    C.check_strided(C.GenCase(*case), SpecOnly())


@pytest.mark.parametrize("case", C.DENSE_STRIDED, ids=C.case_id)
def test_dense_stack_strided_cases(case):
    widths, n, apps, sl = case
    b = SpecOnly()
    assert b.emu.dense_stack_supported(widths) == (widths not in C.DENSE_UNSUPPORTED)
    C.check_strided(C.DenseCase(widths, n, apps, sl), b)  # (the definition does not depend on what fits the LDS)


def test_tile_walk_cases():
    for entry in ("plain", "keep"):
        res = C.GenCase(entry, *C.GEN_WALK_FWD, 0).run(SpecOnly(), True, bwd=False)
        C.assert_finite(res)
    for widths, apps in C.DENSE_WALK:
        b = SpecOnly()
        assert b.emu.dense_stack_supported(widths)
        C.assert_finite(C.DenseCase(widths, C.DENSE_WALK_N[apps], apps).run(b, True))


@pytest.mark.parametrize("enc", [0, 1])
def test_tile_walk_backward_case_and_its_measured_tolerance(enc):
    """The float32 yardstick of the n > 8000 slab sums, re-measured on the case the GPU test runs."""
    case = C.GenCase("plain", *C.GEN_WALK_BWD, enc)
    err = C.f32_error(lambda b: case.run(b, False), ["dw", "db"])
    for nm in ("dw", "db"):
        assert 0 < err[nm] <= C.GEN_WALK_F32_ERR[nm], (nm, err[nm])
    C.assert_finite(C.GenCase("keep", *C.GEN_WALK_BWD, enc).run(SpecOnly(), False))  # (draws its own operands)


def test_band_count_and_width_edge_cases():
    for bands in C.GEN_EDGE_BANDS:
        for n in C.GEN_EDGE_N:
            for enc in (0, 1):
                b = SpecOnly()
                mfma = 16 <= bands <= C.GEN_MFMA_LAST
                assert (b.emu.gan_generator_keep_floats(n, bands, enc) > 0) == mfma
                for entry in ("plain", "keep") if mfma else ("plain",):
                    C.assert_finite(C.GenCase(entry, bands, n, enc).run(b, True))
    b = SpecOnly()
    assert not b.emu.dense_stack_supported((129, 64, 2)) and not b.emu.dense_stack_supported((8, 8, 8, 8, 8, 8))
    for widths in C.DENSE_EDGE:
        assert b.emu.dense_stack_supported(widths)
        for n in C.GEN_EDGE_N:
            C.assert_finite(C.DenseCase(widths, n).run(b, True))


@pytest.mark.parametrize("case", C.GEN_ZERO, ids=C.case_id)
def test_zero_row_cases(case):
    entry, bands, enc = case
    C.assert_finite(C.check_zero_rows(C.GenCase(entry, bands, C.GEN_ZERO_N, enc, zero_rows=True), SpecOnly()))


def test_row_independence_cases():
    for entry, bands in C.GEN_NAN:
        C.check_row_independence(C.GenCase(entry, bands, C.NAN_N, 0), SpecOnly())
    C.check_row_independence(C.DenseCase(C.DENSE_NAN, C.NAN_N), SpecOnly())


def test_valu_child_selection_is_counted_from_the_tables():
    from tests.test_gpu_gan_stacks import valu_child_count
    assert valu_child_count() == 12 + 48 + 5 + 3 + 1


@pytest.mark.parametrize("pe", C.NCE_PE, ids=lambda pe: f"P{pe[0]}E{pe[1]}")
def test_nce_cases(pe):
    for n in C.NCE_N:
        res = C.run_nce(SpecOnly(), *pe, n)
        C.close_all(res, C.NCE_TOL)
        C.assert_finite(res)
    res = C.run_nce(SpecOnly(), *pe, 65, zero_g=True)
    np.testing.assert_allclose(res["loss2"][0][0], 10.0 * pe[0] * np.log(pe[0] ** 2), rtol=1e-6)


@pytest.mark.parametrize("pe", C.NCE_BIG, ids=lambda pe: f"P{pe[0]}E{pe[1]}")
def test_nce_large_logits_case_and_its_measured_tolerance(pe):
    names = [f"{k}{i}" for k in ("loss", "dg", "dr") for i in range(len(C.NCE_STEPS))]
    err = C.f32_error(lambda b: C.run_nce(b, *pe, C.NCE_BIG_N, big=True), names)
    assert 0 < max(err.values()) <= C.NCE_BIG_F32_ERR[pe], err
    C.assert_finite(C.run_nce(SpecOnly(), *pe, C.NCE_BIG_N, big=True))


def test_l2norm_cases_and_the_near_clamp_tolerance():
    worst = 0.0
    for entry, rows, special in C.L2N_CASES:
        C.check_l2norm(SpecOnly(), entry, rows, special)
        if special:
            p = C.l2n_kinds(entry, special).index("tiny")
            err = C.f32_error(lambda b: {k: v for k, v in C.run_l2norm(b, entry, rows, special).items() if k != "_dy"},
                              [f"{k}{p}" for k in ("y", "ss", "inv", "dxa", "dxo")], floor=0.0)
            worst = max(worst, *err.values())
    assert 0 < worst <= C.L2N_TINY_F32_ERR, worst


@pytest.mark.parametrize("rows,c", C.LOSS_SHAPES)
def test_gan_loss_and_slots_cases(rows, c):
    for mode in (0, 1, 2):
        res = C.run_gan_loss(SpecOnly(), mode, rows, c)
        C.close_all(res, C.GAN_LOSS_TOL)
        C.assert_finite(res)
    C.assert_finite(C.run_loss_slots(SpecOnly(), rows, c))


def test_long_regulariser_case_and_its_measured_tolerance():
    err = C.f32_error(lambda b: C.run_loss_slots(b, 1, 1, nw=C.L2_LONG, only_l2=True), ["loss", "dw"])
    for nm in ("loss", "dw"):
        assert err[nm] <= C.L2_LONG_F32_ERR[nm], (nm, err[nm])


# ------------------------------------------------------------------------------- the helpers discriminate (self-checks)
def _spec_output():
    case = C.GenCase("plain", 20, 19, 0)
    b = SpecOnly()
    case.run(b, True)
    a = Arena(19, 20, *C.gen_layout(20)["out"])
    return a, b.e["out"].numpy().copy()


def test_arena_checker_refuses_one_changed_pad_element():
    a, flat = _spec_output()
    off, ld, check, same = arena(19, 20, *C.gen_layout(20)["out"])
    assert (off, ld) == (a.off, a.ld) and same.buf.size == flat.size and a.guard >= 16 * a.ld
    check(flat)
    for where in (a.off - 1, a.off + 20, a.off + 18 * a.ld + 20, 0, flat.size - 1, a.guard - 1, a.guard + 19 * a.ld):
        bad = flat.copy()
        bad[where] = np.nextafter(SENT, np.float32(0))  # one ulp off the sentinel is enough
        with pytest.raises(AssertionError):
            check(bad)
    inside = flat.copy()
    a.window(inside)[3, 4] += 1.0  # a change inside the window is not the checker's business
    check(inside)


def test_bit_identity_refuses_one_ulp():
    a, flat = _spec_output()
    win = a.window(flat).copy()
    assert_same_bits("same", win, win.copy())
    moved = win.copy()
    moved[7, 11] = np.nextafter(moved[7, 11], np.float32(np.inf))
    with pytest.raises(AssertionError):
        assert_same_bits("one ulp", moved, win)
    with pytest.raises(AssertionError):
        assert_same_bits("sign of zero", np.zeros(3, np.float32), -np.zeros(3, np.float32))
    assert_close("one ulp is within any parity tolerance", moved, win, 5e-5, 5e-6)


def test_zero_row_check_refuses_the_other_branch_convention():
    """What a kernel with `c >= 0` would return: the spec run with biases of 1e-30, which puts the zero rows' (otherwise
    exactly zero) pre-activations on the positive side and changes nothing else that float32 can see."""
    case = C.GenCase("plain", 64, C.GEN_ZERO_N, 0, zero_rows=True)
    good = C.check_zero_rows(case, SpecOnly())
    case.bias[:8] = np.float32(1e-30)
    other = case.run(SpecOnly(), False)
    z, rest = case.fixed, np.setdiff1d(np.arange(C.GEN_ZERO_N), case.fixed)
    assert_same_bits("rows off the kink", other["dx"][0][rest], good["dx"][0][rest])
    with pytest.raises(AssertionError):
        assert_close("dx of the zero rows", other["dx"][0][z], good["dx"][1][z], *C.GEN_TOL["plain"]["dx"])
    with pytest.raises(AssertionError):
        assert_close("dx", other["dx"][0], good["dx"][1], *C.GEN_TOL["plain"]["dx"])
