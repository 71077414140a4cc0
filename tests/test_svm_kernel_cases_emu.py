"""CPU: every case table of tests/svm_kernel_cases.py through the numpy twins of the support-vector entry points
(tests/emu_svm.py, tests/emu_svm_grid.py), then the checks are shown to be live: the tables reach what they claim (the
TAU floor, both label relations, the clip outcomes, the l values and both storage paths), defects planted in a copy of
the twin (the tie rule of i and of j, the TAU floor, a clip, the gradient update, the two forms of rho, the sign of
alpha_y) and writes one element outside each output of each solver launch, ws included, must all be rejected."""
import re
from collections import Counter

import numpy as np
import pytest

from tests import svm_kernel_cases as K
from tests.emu_backend import EmuBackend
from tests.emu_svm import mutant  # (the import attaches the twins to EmuBackend)


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.mark.parametrize("group", list(K.SOLVER_GROUPS))
def test_solver_group(emu, group):
    K.run_solver_group(emu, group)


def test_smo_grid(emu):
    K.run_grid(emu)


@pytest.mark.parametrize("name", list(K.value_inputs()))
def test_kernel_values(emu, name):
    K.run_values(emu, name)


@pytest.mark.parametrize("name", ["diagonal", "tail"])
def test_kernel_planes(emu, name):
    K.run_planes(emu, name)


def test_kernel_value_refusals(emu):
    assert len(K.value_refusals(emu)) == 8


@pytest.mark.parametrize("with_labels,with_points", [(False, False), (True, True)])
def test_vote_256_classes(emu, with_labels, with_points):
    K.run_vote(emu, with_labels, with_points)


def test_vote_score_255_classes(emu):
    K.run_vote_score(emu)


def test_tables_cover_what_they_claim():
    """The eighth clip outcome (labels differ, diff <= 0, ai < 0: i of the class y = -1 falls to 0 before j of the class
    y = +1 does) is reachable by second-order selection: l513 takes it once."""
    P = K.problems()
    used = [P[n] for names, _ in K.SOLVER_GROUPS.values() for n in names]
    assert {95, 128, 257, 300, 301, 513, 2048, 2049} <= {q.l for q in used}
    assert K.LDS_L_MAX == 2048 and 3 * 8 * K.LDS_L_MAX == 48 * 1024 and K.WS_L_MAX == 2049  # both storage paths
    assert {q.l for q in used if q.l > K.LDS_L_MAX} == {2049} and K.ROUNDING_GROUPS and K.EXACT_GROUPS
    seen = Counter()
    for group in K.ROUNDING_GROUPS:
        for name in K.SOLVER_GROUPS[group][0]:
            events, steps = P[name].events
            assert steps == P[name].twin[3], name  # the instrumented copy walks the twin's trajectory
            seen.update(events)
    assert seen["tau"] >= 19 and P["copies"].events[0]["tau"] == seen["tau"]
    assert seen["differ"] > 0 and seen["same"] > 0
    assert all(seen[c] > 0 for c in K.CLIPS), {c: seen[c] for c in K.CLIPS}
    assert P["constant"].events[0]["tau"] == 37 and P["negative_curvature"].events[0]["tau"] > 0
    a = np.abs(P["all_at_C"].twin[0])
    assert (a == P["all_at_C"].C).all()  # no free element: rho is (ub + lb) / 2
    free = [int(((np.abs(q.twin[0]) > 0) & (np.abs(q.twin[0]) < q.C)).sum()) for q in (P["rbf95_C0.01"], P["rbf95_C1000"])]
    assert free[0] < 10 and free[1] > 60 and (np.abs(P["rbf95_C1000"].twin[0]) < 1e3).all()  # mostly at bound, all free
    assert set(K.GRID_JOBS) & set(K.SOLVER_GROUPS["tau"][0]) and len(K.GRID_JOBS) == 4
    assert set(K.VALUE_COLS) == {1, 3, 4, 5} and K.VOTE_CLASSES == 256 and K.SCORE_CLASSES == 255


# ------------------------------------------------------------------------------------------------------ planted defects
def test_the_unchanged_copy_passes():
    be = mutant("TAU = 1e-12", "TAU = 1e-12")
    assert be.k_svm_smo_ovo.__func__ is not EmuBackend.k_svm_smo_ovo
    for group in ("identity7", "tau", "C1"):
        K.run_solver_group(be, group)


SECOND_CLIP = """            if diff > 0:
                if ai > C:
                    ai, aj = C, C - diff
            elif aj > C:
                aj, ai = C, C + diff
"""
DEFECTS = {
    "first maximum for i": (("i = _last_argmax(", "i = np.argmax("), ["identity7", "lds_limit"]),
    "first maximum for j": (("j = _last_argmax(", "j = np.argmax("), ["identity7", "lds_limit"]),
    "no TAU floor": (("quad = np.where(quad > 0, quad, TAU)", "quad = quad + 0.0"), ["tau"]),
    "second clip of the opposite-label branch dropped": ((SECOND_CLIP, ""), ["tau", "C1e-2"]),
    "gradient updated from K[i] only": ((" + K[j] * ((aj - aj0) * y[j]))", ")"), ["identity7", "C1"]),
    "rho as the mean over all elements": (("rho = yg[free].sum() / free.sum()", "rho = yg.mean()"), ["identity7", "C1"]),
    "at-bound test of rho swapped": (("at_c, at_0 = alpha >= C, alpha <= 0", "at_c, at_0 = alpha <= C, alpha >= 0"),
                                     ["tau", "C1e-2"]),
    "alpha_y without the sign": (("return alpha * y, rho,", "return alpha, rho,"), ["identity1", "C1e3"]),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_planted_defect_is_rejected(name):
    change, groups = DEFECTS[name]
    be = mutant(*change)
    for group in groups:  # by the exact cases and, where it has a say, by the certificate alone
        with pytest.raises(AssertionError), np.errstate(all="ignore"):
            K.run_solver_group(be, group)


# -------------------------------------------------------------------------------------- writes outside the outputs
class Poking(EmuBackend):
    """the twin, which after launch `launch_no` (both of its runs) zeroes element `elem` of pointer argument `arg`"""

    def __init__(self, launch_no, arg, elem):
        super().__init__()
        self.launch_no, self.arg, self.elem, self.calls = launch_no, arg, elem, 0

    def call(self, name, *args):
        super().call(name, *args)
        if self.calls // 2 == self.launch_no:
            ref = args[self.arg]
            ref.t[ref.off + self.elem] = 0
        self.calls += 1


def outside(op):
    """the element in front of and the one behind every window a launch may write (relative to the pointer)"""
    inside = np.zeros(op.init.size + 2, bool)
    for lo, hi in op.windows:
        inside[lo + 1:hi + 1] = True
    return sorted({e for lo, hi in op.windows for e in (lo - 1, hi) if not inside[e + 1]})


POKE_CASES = {
    "rounding": lambda be: K.run_solver_group(be, "C1e-2"),  # (its second launch: the same problems on the workspace path)
    "exact": lambda be: K.run_solver_group(be, "tau"),
    "grid": lambda be: K.run_grid(be, K.GRID_JOBS_SHORT),
}


@pytest.mark.parametrize("name", list(POKE_CASES))
def test_a_write_one_element_outside_an_output_is_rejected(name):
    recorder = EmuBackend()
    recorder.forest_launches = trace = []  # forest_kernel_cases.launch appends (kernel, args)
    POKE_CASES[name](recorder)
    pokes = []
    for launch_no, (kernel, args) in enumerate(trace):
        for arg, op in enumerate(args):
            if isinstance(op, K.Op) and getattr(op, "windows", None):  # an output
                pokes += [(launch_no, arg, elem, kernel, op.name) for elem in outside(op)]
    outputs = {"alpha_y", "rho", "obj", "n_iter", "status"} | (set() if name == "exact" else {"ws"})  # (exact: LDS only)
    assert {op_name for *_, op_name in pokes} == outputs
    assert len(pokes) >= 10 * len(trace)
    for launch_no, arg, elem, kernel, op_name in pokes:
        with pytest.raises(AssertionError, match=re.escape(f"{kernel} {op_name}")):
            POKE_CASES[name](Poking(launch_no, arg, elem))
