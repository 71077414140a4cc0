"""CPU: every case table of tests/forest_diag_cases.py through the numpy emulation of the forest diagnostics
(tests/emu_forest.py) against the brute-force reference of the case module -- two renditions of include/hypel.h that
share no code.  Then defects planted in a copy of the emulation (a wrong tree filter, the division by n_trees instead of
the votes, the node order of the importance sum reversed, a group taken by division instead of the remainder) must all be
rejected."""
import numpy as np
import pytest

from tests import forest_diag_cases as D
from tests.emu_backend import EmuBackend
from tests.emu_forest import mutant  # (the import attaches the emulation to EmuBackend)


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.mark.parametrize("n,n_classes,n_trees", D.OOB_CASES)
def test_oob_rows(emu, n, n_classes, n_trees):
    D.run_oob(emu, n, n_classes, n_trees)


@pytest.mark.parametrize("case", D.HIT_CASES)
def test_permuted_hits(emu, case):
    D.run_hits(emu, *case)


@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("f", D.IMPORTANCE_F)
def test_importances(emu, f, given):
    D.run_importances(emu, f, given)


def test_importances_lone_roots(emu):
    D.run_importances_lone_roots(emu)


def test_refusals(emu):
    D.run_refusals(emu)
    assert len({(kernel, label) for label, kernel, _ in D.refusal_calls()}) == 31


def test_tables_cover_what_they_claim():
    assert {c[0] for c in D.OOB_CASES} == {c[0] for c in D.HIT_CASES} == {1, 63, 64, 65, 257}
    for table in (D.OOB_CASES, D.HIT_CASES):
        assert {c[1] for c in table} == {2, 32} and {c[2] for c in table} == {1, 3}
    rec, tree_off, _ = D.model_and_rows(0, 4, 2, 3)[1]
    assert tree_off[2] == len(rec) - 1 and rec["left"][-1] < 0  # the third tree is a lone root
    assert {c[3] for c in D.HIT_CASES} >= {1, 3} and {c[4] for c in D.HIT_CASES} >= {1, D.F, 4} and D.F % 4
    assert any(c[5] > 0 for c in D.HIT_CASES)
    assert D.IMPORTANCE_F == [1, 64, D.WINDOW, D.WINDOW + 1]
    rec, tree_off, weight, value, impurity = D.importance_forest(64)
    inner = rec["left"] >= 0
    sizes = np.diff(np.concatenate([tree_off, [len(rec)]]))
    assert (inner[:sizes[0]].sum() > D.BLOCK) and len(set(rec["feature"][:sizes[0]][inner[:sizes[0]]])) == 1
    assert sizes[1] > 2 * D.BLOCK and sizes[2] == 1


# ------------------------------------------------------------------------------------------------------ planted defects
def test_the_unchanged_copy_passes():
    be = mutant("~(in_bag > 0)", "~(in_bag > 0)")
    assert be.k_forest_oob_rows.__func__ is not EmuBackend.k_forest_oob_rows
    D.run_oob(be, 65, 2, 1)
    D.run_hits(be, *D.HIT_CASES[3])
    D.run_importances(be, 64, True)
    D.run_hits_tree_order(be)


DEFECTS = {
    "trees with a count of 1 vote": (("~(in_bag > 0)", "~(in_bag > 1)"), lambda be: D.run_oob(be, 63, 2, 3)),
    "the in-bag trees vote": (("~(in_bag > 0)", "(in_bag > 0)"), lambda be: D.run_oob(be, 63, 2, 3)),
    "divided by n_trees, not the votes": (("np.divide(total, votes[:, None].astype(np.float64)",
                                           "np.divide(total, np.float64(ends.shape[0])"),
                                          lambda be: D.run_oob(be, 64, 32, 3)),
    "node order of the importance sum reversed": (("at = at[l[at] >= 0]", "at = at[l[at] >= 0][::-1]"),
                                                  lambda be: D.run_importances(be, 64, True)),
    "the mean over all trees": (("mean = total / np.float64(used)", "mean = total / np.float64(n_trees)"),
                                lambda be: D.run_importances(be, 64, False)),
    "group by division": (("np.arange(f) % group_mod == g", "np.arange(f) // group_mod == g"),
                          lambda be: D.run_hits(be, *D.HIT_CASES[3])),
    "hits overwritten": (("h[g - g0, r] += int(", "h[g - g0, r] = int("), lambda be: D.run_hits(be, *D.HIT_CASES[2])),
}
# the walk and the vote are shared with serving (tests/test_forest_kernel_cases_emu.py plants the same three there):
# (change, what rejects it out of bag, what rejects it in the permuted hits)
WALK_DEFECTS = {
    "reverse tree order in the fp64 sum": (("for t in range(ends.shape[0]):", "for t in reversed(range(ends.shape[0])):"),
                                           lambda be: D.run_oob(be, 64, 32, 3), D.run_hits_tree_order),
    "threshold compare < instead of <=": (("feature[at]) <= threshold[at]", "feature[at]) < threshold[at]"),
                                          lambda be: D.run_oob(be, 63, 2, 3), lambda be: D.run_hits(be, *D.HIT_CASES[2])),
    "last-maximum vote": (("np.argmax(mean, 1)", "mean.shape[1] - 1 - np.argmax(mean[:, ::-1], 1)"),
                          lambda be: D.run_oob(be, 63, 2, 3), lambda be: D.run_hits(be, *D.HIT_CASES[2])),
}
for _name, (_change, _oob, _hits) in WALK_DEFECTS.items():
    DEFECTS[f"{_name} (out-of-bag)"], DEFECTS[f"{_name} (permuted hits)"] = (_change, _oob), (_change, _hits)


@pytest.mark.parametrize("name", list(DEFECTS))
def test_planted_defect_is_rejected(name):
    change, runner = DEFECTS[name]
    with pytest.raises((AssertionError, ZeroDivisionError, FloatingPointError)):
        runner(mutant(*change))
