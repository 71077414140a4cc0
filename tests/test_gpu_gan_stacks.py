"""-m gpu: the fused generator (csrc/gan_mfma.hip, csrc/gan.hip) and the fused dense stack (csrc/dense_stack.hip) through
the C-ABI against the float64 spec (tests/emu_backend.py), called the way the planner calls them: every row operand a
slice with its own leading dimension and column offset inside a sentinel-filled allocation (tests/parity_util.Arena), so
that a wrong address shows as a broken sentinel or a bit that differs from the contiguous launch -- one failing assertion
at the kernel, not a drifting loss curve.  Cases and checks: tests/gan_kernel_cases.py (the same run through the spec
alone in tests/test_gan_kernel_cases_emu.py).  Groups: g1 strided slices, g2 tile walks, g3 band-count and width edges,
g4 branch convention at zero, g5 row independence, g6 the VALU kernels in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hypelcnn_amd.backend import HypelError, Ref
from tests import gan_kernel_cases as C
from tests.parity_util import SENT, Both, assert_same_bits, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


# ---------------------------------------------------------------------------------------------------- 1. strided slices
@pytest.mark.parametrize("case", C.GEN_STRIDED, ids=C.case_id)
def test_g1_generator_strided(hip, case):
    """(a) spec parity at the tolerance of the entry point's existing test, (b) bit identity with the contiguous launch
    (out, dx, enc_out, every slab), (c) sentinels, (d) both accumulate_dx flags on a pre-filled dx, (e) dx = NULL."""
    C.check_strided(C.GenCase(*case), Both(hip))


@pytest.mark.parametrize("case", C.DENSE_STRIDED, ids=C.case_id)
def test_g1_dense_stack_strided(hip, case):
    widths, n, apps, sl = case
    dc = C.DenseCase(widths, n, apps, sl)
    assert hip.dense_stack_supported(widths) == (widths not in C.DENSE_UNSUPPORTED)
    if widths in C.DENSE_UNSUPPORTED:  # (gan_kernel_cases.DENSE_UNSUPPORTED: why) refused, and nothing is launched
        b = Both(hip)
        with pytest.raises(HypelError):
            dc.run(b, True, bwd=False)
        hip.synchronize()
        assert (bits(b.h["out"].cpu().numpy()) == bits(SENT)).all()
        with pytest.raises(HypelError):
            dc.run(b, True, fwd=False)
        hip.synchronize()
        assert (bits(b.h["pw"].cpu().numpy()) == bits(SENT)).all() and (bits(b.h["pb"].cpu().numpy()) == bits(SENT)).all()
        assert_same_bits("dx", b.h["dx"].cpu().numpy(), C.Arena(apps * n, widths[0], *dc.lay["dx"], dc.dx0).buf)
        return
    C.check_strided(dc, Both(hip))


# --------------------------------------------------------------------------------------------------------- 2. tile walks
@pytest.mark.parametrize("entry", ["plain", "keep"])
def test_g2_generator_forward_walks_two_tiles(hip, entry):
    """16 bands, n = 16 * 1024 + 16 + 5: a grid of 1024 blocks, two of them walk two row tiles, the last tile has 5 rows."""
    bands, n = C.GEN_WALK_FWD
    assert 2 * hip.gan_generator_blocks(n) == 1024 and (n + 15) // 16 == 1026
    case = C.GenCase(entry, bands, n, 0)
    res = case.run(Both(hip), True, bwd=False)
    case.parity(res)


@pytest.mark.parametrize("entry,enc", [("plain", 0), ("keep", 0), ("plain", 1), ("keep", 1)])
def test_g2_generator_backward_walks_two_tiles(hip, entry, enc):
    """48 bands, n = 8192 + 16 + 3: the recomputing and the kept backward, each against the spec (not against each other),
    512 blocks of which two walk two tiles; the slab-summed dw / db against the spec.

    dw / db are sums over n > 8000 samples, more than any existing test compares with the spec: their tolerance is
    measured, not guessed.  A float32 NumPy evaluation of the same formulas lies within 8.3e-7 (dw) and 3.4e-6 (db) of
    max(1, max|spec|) of the float64 spec (largest of three draws per case, gan_kernel_cases.GEN_WALK_F32_ERR); the
    device is allowed 4 x that: 3.3e-6 and 1.4e-5.  out and dx are per-row quantities: the existing tolerances."""
    bands, n = C.GEN_WALK_BWD
    assert hip.gan_generator_blocks(n) == 512 and (n + 15) // 16 == 514
    case = C.GenCase(entry, bands, n, enc)
    res = case.run(Both(hip), False)
    for nm in ("dw", "db"):
        print(f"{entry} enc={enc} {nm}: max |device - spec| / max(1, max|spec|) =",
              np.abs(res[nm][0] - res[nm][1]).max() / max(1.0, np.abs(res[nm][1]).max()))
    case.parity(res, tol={nm: C.measured_tol(C.GEN_WALK_F32_ERR[nm]) for nm in ("dw", "db")})


@pytest.mark.parametrize("case", C.DENSE_WALK, ids=C.case_id)
def test_g2_dense_stack_walks_several_tiles(hip, case):
    """n = 4096 + 16 + 3 (2048 + 16 + 3 per application): blocks walk two tiles, the input is narrower than the hidden
    layers (stale LDS margins of the previous tile's wider layer would show), the last tile is ragged after a full one.
    Slab sums at these n are within what test_dense_stack_fwd_bwd already compares with the spec (n = 5000)."""
    widths, apps = case
    assert hip.dense_stack_supported(widths)
    dc = C.DenseCase(widths, C.DENSE_WALK_N[apps], apps)
    dc.parity(dc.run(Both(hip), True))


# ------------------------------------------------------------------------------------------ 3. band-count / width edges
@pytest.mark.parametrize("n", C.GEN_EDGE_N)
@pytest.mark.parametrize("bands", C.GEN_EDGE_BANDS)
def test_g3_generator_band_counts(hip, bands, n):
    """keep_floats is 0 exactly where the matrix cores are not used; where they are, the kept pair runs as well."""
    mfma = 16 <= bands <= C.GEN_MFMA_LAST
    for enc in (0, 1):
        assert (hip.gan_generator_keep_floats(n, bands, enc) > 0) == mfma
        assert bool(hip.gan_generator_tap_supported(bands)) == mfma
        for entry in ("plain", "keep") if mfma else ("plain",):
            case = C.GenCase(entry, bands, n, enc)
            res = case.run(Both(hip), True)
            case.parity(res)
            C.assert_finite(res)


def test_g3_generator_512_bands_is_refused(hip):
    """The backward pass of 512 bands fits neither VALU kernel's LDS: an error, and nothing is launched (dx, the slabs
    keep their sentinels).  The forward pass alone still fits the register-tiled kernel and is held to the spec."""
    bands, n = 512, 9
    fwd = C.GenCase("plain", bands, n, 0)
    fwd.parity(fwd.run(Both(hip), True, bwd=False))
    wt = sum(C.gen_ks(bands))
    blocks = hip.gan_generator_blocks(n)
    x = hip.upload(np.random.default_rng(0).random((n, bands)).astype(np.float32))
    w, b = hip.upload(np.zeros(wt, np.float32)), hip.upload(np.zeros(8, np.float32))
    dx, pw, pb = (hip.upload(np.full(k, SENT, np.float32)) for k in (n * bands, blocks * wt, blocks * 8))
    with pytest.raises(HypelError):
        hip.call("gan_generator_bwd", Ref(x), bands, Ref(x), bands, n, bands, Ref(w), Ref(b), 0, Ref(dx), bands, 0, Ref(pw),
                 Ref(pb))
    hip.synchronize()
    for t in (dx, pw, pb):
        assert (bits(t.cpu().numpy()) == bits(SENT)).all()
    assert hip.gan_generator_keep_floats(n, bands, 0) == 0 and not hip.gan_generator_tap_supported(bands)


@pytest.mark.parametrize("n", C.GEN_EDGE_N)
@pytest.mark.parametrize("widths", C.DENSE_EDGE, ids=lambda w: "x".join(map(str, w)))
def test_g3_dense_stack_widths(hip, widths, n):
    assert hip.dense_stack_supported(widths)
    assert not hip.dense_stack_supported((129, 64, 2)) and not hip.dense_stack_supported((64, 129, 2))
    assert not hip.dense_stack_supported((64, 64, 129)) and not hip.dense_stack_supported((8, 8, 8, 8, 8, 8))
    assert not hip.lib.hypel_dense_stack_supported(5, 8, 8, 8, 8, 8)
    dc = C.DenseCase(widths, n)
    res = dc.run(Both(hip), True)
    dc.parity(res)
    C.assert_finite(res)


# ---------------------------------------------------------------------------------------- 4. branch convention at zero
@pytest.mark.parametrize("case", C.GEN_ZERO, ids=C.case_id)
def test_g4_generator_zero_preactivations_take_the_small_slope(hip, case):
    """No biases, every other row of x exactly zero: every pre-activation of those rows is exactly 0 in fp32 and float64,
    and the branch `c > 0` takes slope 0.1 -- in the forward pass, the recomputing backward and the kept branch bits."""
    entry, bands, enc = case
    C.check_zero_rows(C.GenCase(entry, bands, C.GEN_ZERO_N, enc, zero_rows=True), Both(hip))


# ------------------------------------------------------------------------------------------------- 5. row independence
@pytest.mark.parametrize("case", C.GEN_NAN, ids=C.case_id)
def test_g5_generator_rows_are_independent(hip, case):
    entry, bands = case
    C.check_row_independence(C.GenCase(entry, bands, C.NAN_N, 0), Both(hip))


def test_g5_dense_stack_rows_are_independent(hip):
    C.check_row_independence(C.DenseCase(C.DENSE_NAN, C.NAN_N), Both(hip))


# ----------------------------------------------------------------------------------------------------- 6. VALU kernels
def valu_child_count():
    """what `-k "(g1 or g4 or g5) and not mfma_only"` selects of this file"""
    return (sum(c[0] not in C.MFMA_ONLY for c in C.GEN_STRIDED) + len(C.DENSE_STRIDED)
            + sum(c[0] not in C.MFMA_ONLY for c in C.GEN_ZERO) + sum(c[0] not in C.MFMA_ONLY for c in C.GEN_NAN) + 1)


def test_g6_valu_kernels_in_a_subprocess():
    """HYPEL_GAN_MFMA=0 (read once per process): groups 1, 4 and 5 once more on gan.hip's wave-per-sample and
    register-tiled kernels -- without the entry points that exist on the matrix cores only."""
    env = dict(os.environ, HYPEL_GAN_MFMA="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "(g1 or g4 or g5) and not mfma_only", "-p", "no:cacheprovider"], env=env, capture_output=True,
                       text=True, timeout=240, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"{valu_child_count()} passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
