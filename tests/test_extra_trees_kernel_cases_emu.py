"""CPU: every case table of tests/extra_trees_kernel_cases.py through the numpy emulation of the extra-trees entry points
(tests/emu_extra_trees.py) against the brute-force reference of the case module -- two renditions of include/hypel.h that
share no code.  Then defects planted in a copy of the emulation (the fallback of the cut dropped, `<` for `<=` in the
partition, the column order of a score tie reversed, the sign of zero kept) must all be rejected."""
import inspect

import pytest

from tests import emu_extra_trees
from tests import emu_forest  # noqa: F401 -- (the gather and serving twins the shared helpers may call)
from tests import extra_trees_kernel_cases as X
from tests.emu_backend import EmuBackend


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
    X.run_partition(emu)


@pytest.mark.parametrize("level,max_depth", X.LEAF_LEVELS)
def test_split_apply_thr_leaf_reasons(emu, level, max_depth):
    X.run_leaf_reasons(emu, level, max_depth)


def test_split_apply_thr_slot_ties(emu):
    X.run_slot_ties(emu)


@pytest.mark.parametrize("n_active", X.COMPACT_N)
def test_split_apply_thr_compaction(emu, n_active):
    for pattern in X.COMPACT_PATTERNS:
        X.run_compaction(emu, n_active, pattern)
    X.run_compaction(emu, n_active, "alternating", short=1)
    X.run_compaction(emu, n_active, "last", short=1)


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
    assert min(X.PART_COUNTS) == 2 and max(X.PART_COUNTS) == 1000


# ------------------------------------------------------------------------------------------------------ planted defects
def mutant(old, new):
    """EmuBackend with the entry points of a copy of tests/emu_extra_trees.py in which `old` reads `new`"""
    src = inspect.getsource(emu_extra_trees).split("\nfor _name, _fn in")[0]
    assert src.count(old) == 1, (old, src.count(old))
    ns = {"__name__": "emu_extra_trees_mutant"}
    exec(compile(src.replace(old, new), "<emu_extra_trees mutant>", "exec"), ns)
    return type("Mutant", (EmuBackend,), {k[1:]: v for k, v in ns.items() if k.startswith("_k_forest_")})()


def test_the_unchanged_copy_passes():
    be = mutant("if not (t < hi):", "if not (t < hi):")
    assert be.k_forest_split_random.__func__ is not EmuBackend.k_forest_split_random
    X.run_random_special(be)
    X.run_slot_ties(be)
    X.run_partition(be)
    X.run_columns(be, 63, 5)


DEFECTS = {
    "the fallback of the cut dropped": (("    if not (t < hi):\n        t = lo\n", ""), X.run_random_special),
    "partition by < instead of <=": (("go_left = cols[c][rows] <= t", "go_left = cols[c][rows] < t"), X.run_partition),
    "the higher column on a score tie": (("key=lambda k: (-sc[a, k], cd[a, k])", "key=lambda k: (-sc[a, k], -cd[a, k])"),
                                         X.run_slot_ties),
    "counted by < instead of <=": (("cut_score(v <= t,", "cut_score(v < t,"), lambda be: X.run_random(be, "c3_w9")),
    "the sign of zero kept": ((".T + np.float32(0)", ".T"), lambda be: X.run_columns(be, 63, 5)),
    "level > max_depth": (("or level >= max_depth", "or level > max_depth"), lambda be: X.run_leaf_reasons(be, 4, 4)),
    "thr_bin of a split node written": (("out[\"feature\"][node], tv[node] = c, t",
                                         "out[\"feature\"][node], tv[node], out[\"thr_bin\"][node] = c, t, 0"),
                                        X.run_slot_ties),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_planted_defect_is_rejected(name):
    change, runner = DEFECTS[name]
    with pytest.raises((AssertionError, ZeroDivisionError, FloatingPointError)):
        runner(mutant(*change))
