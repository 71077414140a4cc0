"""GPU: the scene-side and classic-ML launches past one pass of their capped grid -- the cases of
tests/grid_pass_cases.py at big=True, the smallest size of each that takes a second trip of the grid-stride loop plus an
odd tail.  Every output sits in a sentinel-filled buffer that is compared whole; everything is compared exactly but the
kernel values (2^-23 relative, test_kernel_apply_vs_float64's bound) and the row norms (1e-12 of the largest,
test_center_norms_vs_float64's); a launch that uses atomics runs twice and must give the same bytes."""
import time

import pytest

from tests import grid_pass_cases as G
from tests import head_kernel_cases as H
from tests import parity_util as PU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_second_trip(be, case):
    t0 = time.perf_counter()
    built = case.build(True)
    for what, ok in built.facts:
        assert ok, f"{case.name}: {what}"
    for name, ex in built.expect.items():  # a tail nobody writes cannot pass
        assert ex.late_outputs_differ()[1] == 0, f"{case.name} {name}: late outputs equal the pre-fill"
    t1 = time.perf_counter()
    got = built.run(be)
    t2 = time.perf_counter()
    G.compare(case.name, built, got)
    if case.twice:
        again = built.run(be)
        for name in got:
            G.same_bytes(f"{case.name} {name}, second run", again[name], got[name])
    if case.twin:
        import tests.emu_svm_grid  # noqa: F401 -- the twin of hypel_svm_scatter_coef_f32
        from tests.emu_backend import EmuBackend
        twin = built.run(EmuBackend())
        for name in got:
            G.same_bytes(f"{case.name} {name}, the twin", twin[name], got[name])
    print(f"{case.name}: pass {case.pass_items}, items {case.items(True)}, reference {t1 - t0:.2f} s, device run with "
          f"transfers {t2 - t1:.2f} s, all {time.perf_counter() - t0:.2f} s")


def test_patch_walks(be):
    """hypel_gather_patches_2x_f32 and hypel_augment_patches_f32 past 8192 patch pixels, one block each"""
    H.run_gather_2x(PU.Both(be), **G.GATHER_2X_WALK)
    H.run_augment(PU.Both(be), **G.AUGMENT_WALK)
