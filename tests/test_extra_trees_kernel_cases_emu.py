"""CPU: every case table of tests/extra_trees_kernel_cases.py through the numpy emulation of the extra-trees entry points
(tests/emu_forest.py) against the brute-force reference of the case module -- two renditions of include/hypel.h that
share no code.  Then defects planted in a copy of the emulation (the fallback of the cut dropped, `<` for `<=` in the
partition, the column order of a score tie reversed, the sign of zero kept) must all be rejected."""
import pytest

from tests import extra_trees_kernel_cases as X
from tests import forest_kernel_cases as K
from tests.emu_backend import EmuBackend
from tests.emu_forest import mutant  # (the import attaches the emulation to EmuBackend)


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.mark.parametrize("n,f", X.COLUMN_CASES)
def test_columns(emu, n, f):
    X.run_columns(emu, n, f)


@pytest.mark.parametrize("name", list(X.RANDOM_CASES))
def test_split_random(emu, name):
    X.run_random(emu, name)


def test_split_random_special_columns(emu):
    X.run_random_special(emu)


def test_split_apply_thr_partition(emu):
    K.run_partition(emu, K.CUTS)


@pytest.mark.parametrize("level,max_depth", K.LEAF_LEVELS)
def test_split_apply_thr_leaf_reasons(emu, level, max_depth):
    K.run_leaf_reasons(emu, K.CUTS, level, max_depth)


def test_split_apply_thr_slot_ties(emu):
    K.run_slot_ties(emu, K.CUTS)


@pytest.mark.parametrize("n_active", K.COMPACT_N)
def test_split_apply_thr_compaction(emu, n_active):
    for pattern in K.COMPACT_PATTERNS:
        K.run_compaction(emu, K.CUTS, n_active, pattern)
    K.run_compaction(emu, K.CUTS, n_active, "alternating", short=1)
    K.run_compaction(emu, K.CUTS, n_active, "last", short=1)


@pytest.mark.parametrize("name", ["600_nodes", "c32_mff"])
def test_split_random_then_apply(emu, name):
    X.run_random_then_apply(emu, name)


def test_refusals(emu):
    X.run_refusals(emu)
    assert len({(kernel, label) for label, kernel, _ in X.refusal_calls()}) == 14


def test_tables_cover_what_they_claim():
    assert X.COLUMN_CASES == [(1, 1), (63, 5), (65, 33), (257, 3)]
    assert set(X.ROW_COUNTS) == {1, 2, 63, 64, 65, 256, 257, 1000}
    assert {c[1] for c in X.RANDOM_CASES.values()} >= {2, 32} and {c[2] for c in X.RANDOM_CASES.values()} >= {1, 5}
    d, cand, _ = X.random_scenario("c32_mff")
    assert cand.shape[1] == d["f"] and d["weight"].max() > 1
    d, cand, _ = X.random_scenario("600_nodes")
    assert d["n_active"] == 600 and {len(s) for s in d["segs"]} == set(range(2, 9))
    assert min(K.PART_COUNTS) == 2 and max(K.PART_COUNTS) == 1000


# ------------------------------------------------------------------------------------------------------ planted defects
def test_the_unchanged_copy_passes():
    be = mutant("if not (t < hi):", "if not (t < hi):")
    assert be.k_forest_split_random.__func__ is not EmuBackend.k_forest_split_random
    X.run_random_special(be)
    K.run_slot_ties(be, K.CUTS)
    K.run_partition(be, K.CUTS)
    X.run_columns(be, 63, 5)


DEFECTS = {
    "the fallback of the cut dropped": (("    if not (t < hi):\n        t = lo\n", ""), X.run_random_special),
    "partition by < instead of <=": (("go_left = table[c][rows] <= cut[a, s]", "go_left = table[c][rows] < cut[a, s]"),
                                     lambda be: K.run_partition(be, K.CUTS)),
    "the higher column on a score tie": (("key=lambda k: (-sc[a, k], cd[a, k])", "key=lambda k: (-sc[a, k], -cd[a, k])"),
                                         lambda be: K.run_slot_ties(be, K.CUTS)),
    "counted by < instead of <=": (("cut_score(v <= t,", "cut_score(v < t,"), lambda be: X.run_random(be, "c3_w9")),
    "the sign of zero kept": ((".T + np.float32(0)", ".T"), lambda be: X.run_columns(be, 63, 5)),
    "level > max_depth": (("or level >= max_depth", "or level > max_depth"), lambda be: K.run_leaf_reasons(be, K.CUTS, 4, 4)),
    "thr_bin of a split node written": (("thr_bin[node], threshold[node] = -1, t", "thr_bin[node], threshold[node] = 0, t"),
                                        lambda be: K.run_slot_ties(be, K.CUTS)),
    "unstable partition": (("np.concatenate([rows[go_left], rows[~go_left]])",
                            "np.concatenate([rows[go_left][::-1], rows[~go_left]])"), lambda be: K.run_partition(be, K.CUTS)),
    "a child may take node_capacity": (("if lid + 1 < node_capacity:", "if lid + 1 <= node_capacity:"),
                                       lambda be: K.run_compaction(be, K.CUTS, 257, "alternating", short=1)),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_planted_defect_is_rejected(name):
    change, runner = DEFECTS[name]
    with pytest.raises((AssertionError, ZeroDivisionError, FloatingPointError)):
        runner(mutant(*change))
