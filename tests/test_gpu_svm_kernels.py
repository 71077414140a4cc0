"""-m gpu: the kernels of csrc/svm.hip through the C-ABI (HipBackend.call), one entry point at a time, by the runners of
tests/svm_kernel_cases.py.  The solver (svm_smo_solve, behind hypel_svm_smo_ovo and hypel_svm_smo_grid) is held to an
optimality certificate recomputed in np.longdouble where its arithmetic rounds, and byte for byte to closed forms and to
the numpy twin where every intermediate is an integer or a small dyadic; the kernel values to float64 within half an fp32
ulp; the votes to the twin's at 256 and 255 classes.  tests/test_svm_kernel_cases_emu.py runs the same runners through the
twins on the CPU and shows that planted defects and stray writes are rejected.

Every operand lies at an odd element offset inside sentinel bytes; every launch runs twice from fresh uploads and must write
the same bytes; after it K, the tables, the gaps of alpha_y, the slots past the last problem, the workspace outside each
pair's own part and every guard must hold what they held."""
import pytest

from tests import svm_kernel_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.mark.parametrize("group", K.ROUNDING_GROUPS)
def test_s1_solver_certificate(hip, group):
    """RBF and polynomial problems of l = 90 .. 513 (C from 1e-2, every multiplier at C, to 1e3, every one free; a class
    of one row; exact copies across the classes, whose curvature is 0), several pairs per launch: the certificate, and
    the workspace path (l_max = 2049) bit for bit the LDS path.  Prints gap - tol and the iterations beside the twin's."""
    K.run_solver_group(hip, group)


@pytest.mark.parametrize("group", K.EXACT_GROUPS)
def test_s2_solver_exact(hip, group):
    """K = I after 1, 7, 130 and (l = 2048, the last that fits LDS; l = 2049, refused without a workspace) 64 steps, K = 1
    and a K of negative curvature: alpha_y, rho, obj, n_iter and status byte for byte the closed form and the twin"""
    K.run_solver_group(hip, group)


def test_s3_smo_grid(hip):
    """exact and rounding problems as the jobs of one launch, two planes, own c and k_off, permuted order, both storage
    paths: every job bit for bit its own hypel_svm_smo_ovo launch"""
    K.run_grid(hip)


@pytest.mark.parametrize("name", list(K.value_inputs()))
def test_s4_kernel_values(hip, name):
    """self-products either side of the clamp, exponents down to denormal and zero results, degrees 1 to 3, values beyond
    FLT_MAX; the vector form, the scalar forms (a base one float off 16 bytes, an odd ld) on 1, 3, 4 and 5 columns"""
    K.run_values(hip, name)


@pytest.mark.parametrize("name", ["diagonal", "tail"])
def test_s4_kernel_planes(hip, name):
    K.run_planes(hip, name)


def test_s4_kernel_value_refusals_leave_every_byte(hip):
    K.value_refusals(hip)


@pytest.mark.parametrize("with_labels,with_points", [(False, False), (True, True)])
def test_s5_vote_256_classes(hip, with_labels, with_points):
    """65 536 bytes of counters per block; classes with all 255 votes, rows of NaN and of -0.0"""
    K.run_vote(hip, with_labels, with_points)


def test_s5_vote_score_255_classes(hip):
    K.run_vote_score(hip)
