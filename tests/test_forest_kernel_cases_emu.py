"""CPU: every case table of tests/forest_kernel_cases.py through the numpy emulation of the forest entry points
(tests/emu_forest.py) against the brute-force reference of the case module -- two renditions of include/hypel.h that
share no code, so a disagreement means one of them misreads the header.  Then the checks are shown to be live: defects
planted in a copy of the emulation (the bin search, the tie rules, the partition, the sums of squares, the vote, the
order of the fp64 sum) and writes one element outside each output must all be rejected."""
import re

import numpy as np
import pytest

from tests import forest_kernel_cases as K
from tests.emu_backend import EmuBackend
from tests.emu_forest import mutant  # (the import attaches the emulation to EmuBackend)


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.mark.parametrize("k,case", list(enumerate(K.BIN_CASES)), ids=[f"{n}x{b}" for n, b in K.BIN_CASES])
def test_bin_edges_and_bins(emu, k, case):
    K.run_bins(emu, *case, k)


@pytest.mark.parametrize("name", list(K.HIST_CASES))
def test_split_hist(emu, name):
    K.run_hist(emu, name)


def test_split_apply_partition(emu):
    K.run_partition(emu, K.BINS)


@pytest.mark.parametrize("level,max_depth", K.LEAF_LEVELS)
def test_split_apply_leaf_reasons(emu, level, max_depth):
    K.run_leaf_reasons(emu, K.BINS, level, max_depth)


def test_split_apply_slot_ties(emu):
    K.run_slot_ties(emu, K.BINS)


@pytest.mark.parametrize("n_active", K.COMPACT_N)
def test_split_apply_compaction(emu, n_active):
    for pattern in K.COMPACT_PATTERNS:
        K.run_compaction(emu, K.BINS, n_active, pattern)
    K.run_compaction(emu, K.BINS, n_active, "alternating", short=1)
    K.run_compaction(emu, K.BINS, n_active, "last", short=1)


@pytest.mark.parametrize("name", ["c2_mf1", "heavy_c32", "special"])
def test_split_hist_then_apply(emu, name):
    K.run_hist_then_apply(emu, name)


@pytest.mark.parametrize("n,n_classes,n_trees", K.PREDICT_CASES)
def test_predict_rows(emu, n, n_classes, n_trees):
    K.run_predict(emu, n, n_classes, n_trees)


def test_predict_rows_ties_and_thresholds(emu):
    K.run_predict_ties(emu)
    K.run_predict_threshold(emu)


@pytest.mark.parametrize("p,cc,cl,n", K.SCENE_CASES)
def test_predict_scene(emu, p, cc, cl, n):
    K.run_scene(emu, p, cc, cl, n)


def test_refusals(emu):
    K.run_refusals(emu)
    labels = {(kernel, label) for label, kernel, _ in K.refusal_calls()}
    assert len(labels) == 23


def test_tables_cover_what_they_claim():
    assert {n for n, _ in K.BIN_CASES} == {1, 2, 3, 255, 1023, 1024, 1025, 16384, 16385}
    assert {b for _, b in K.BIN_CASES} == {2, 3, 255, 256} and any(n < b for n, b in K.BIN_CASES)
    assert set(K.PROBE_N) == {1, 255, 256, 257, 513} and len(K.BIN_CASES) >= len(K.PROBE_N)
    assert {c[1] for c in K.HIST_CASES.values()} == {1, 2, 15, 32} and {c[2] for c in K.HIST_CASES.values()} == {1, 3, 5}
    assert {1, 5, 300} <= {len(K.hist_scenario(name)[1]) for name in K.HIST_CASES}
    assert {n for n, _, _ in K.PREDICT_CASES} == {1, 63, 64, 65, 130}
    assert {c for _, c, _ in K.PREDICT_CASES} == {1, 2, 32} and {t for _, _, t in K.PREDICT_CASES} == {1, 3, 50}


# ------------------------------------------------------------------------------------------------------ planted defects
def test_the_unchanged_copy_passes():
    be = mutant("side=\"left\"", "side=\"left\"")
    assert be.k_forest_bin_u8.__func__ is not EmuBackend.k_forest_bin_u8
    K.run_bins(be, 3, 256)
    K.run_slot_ties(be, K.BINS)
    K.run_predict_ties(be)


DEFECTS = {
    "bin search <= instead of <": (("side=\"left\"", "side=\"right\""), lambda be: K.run_bins(be, 255, 256)),
    "edge at the column maximum kept": (("if v >= s[-1]:", "if v > s[-1]:"), lambda be: K.run_bins(be, 2, 3)),
    "highest bin on a tie": (("t = int(np.argmax(sc))", "t = E - 1 - int(np.argmax(sc[::-1]))"),
                             lambda be: K.run_hist(be, "special")),
    "int32 sums of squares": (("sl, sr = (left * left).sum(1), (right * right).sum(1)",
                               "sl, sr = (left * left).sum(1).astype(np.int32), (right * right).sum(1).astype(np.int32)"),
                              lambda be: K.run_hist(be, "heavy_c2")),
    "rows of weight 0 make a side non-empty": (("nl, nr = left.sum(1), right.sum(1)",
                                                "nl, nr = np.maximum(left.sum(1), 1), np.maximum(right.sum(1), 1)"),
                                               lambda be: K.run_hist(be, "special")),
    "slot order on a slot tie": (("key=lambda k: (-sc[a, k], cd[a, k]) + tie(a, k)", "key=lambda k: (-sc[a, k], k)"),
                                 lambda be: K.run_slot_ties(be, K.BINS)),
    "unstable partition": (("np.concatenate([rows[go_left], rows[~go_left]])",
                            "np.concatenate([rows[go_left][::-1], rows[~go_left]])"), lambda be: K.run_partition(be, K.BINS)),
    "partition by < instead of <=": (("go_left = table[c][rows] <= cut[a, s]", "go_left = table[c][rows] < cut[a, s]"),
                                     lambda be: K.run_partition(be, K.BINS)),
    "level > max_depth": (("or level >= max_depth", "or level > max_depth"), lambda be: K.run_leaf_reasons(be, K.BINS, 4, 4)),
    "a child may take node_capacity": (("if lid + 1 < node_capacity:", "if lid + 1 <= node_capacity:"),
                                       lambda be: K.run_compaction(be, K.BINS, 257, "alternating", short=1)),
    "last-maximum vote (rows)": (("np.argmax(mean, 1)", "mean.shape[1] - 1 - np.argmax(mean[:, ::-1], 1)"),
                                 lambda be: K.run_predict_ties(be)),
    "last-maximum vote (scene)": (("np.argmax(mean, 1)", "mean.shape[1] - 1 - np.argmax(mean[:, ::-1], 1)"),
                                  lambda be: K.run_scene(be, 3, 2, 2, 65)),
    "reverse tree order in the fp64 sum": (("for t in range(ends.shape[0]):", "for t in reversed(range(ends.shape[0])):"),
                                           lambda be: K.run_predict_ties(be)),
    "threshold compare < instead of <=": (("feature[at]) <= threshold[at]", "feature[at]) < threshold[at]"),
                                          lambda be: K.run_predict_threshold(be)),
    "lidar read for casi": (("e, which = code >> 1, code & 1", "e, which = code >> 1, 1 - (code & 1)"),
                            lambda be: K.run_scene(be, 3, 2, 2, 65)),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_planted_defect_is_rejected(name):
    change, runner = DEFECTS[name]
    with pytest.raises(AssertionError):
        runner(mutant(*change))


# -------------------------------------------------------------------------------------- writes outside the outputs
class Poking(EmuBackend):
    """the emulation, which after launch `launch_no` (both of its runs) zeroes element `elem` of pointer argument `arg`"""

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
    """elements just outside what the reference wrote of an output (relative to the pointer): the one in front of the
    operand, the one behind it, and the first and last untouched sentinel that has a written neighbour"""
    item = op.want.itemsize
    untouched = (op.want.view(np.uint8).reshape(-1, item) == K.FILL).all(1)
    edge = untouched & ~(np.r_[True, untouched[:-1]] & np.r_[untouched[1:], True])
    inner = np.flatnonzero(edge)
    return [-1, op.want.size] + ([int(inner[0]), int(inner[-1])] if inner.size else [])


POKE_CASES = {
    "bins": lambda be: K.run_bins(be, 3, 256),
    "split_hist": lambda be: K.run_hist(be, "one_node"),
    "leaf_reasons": lambda be: K.run_leaf_reasons(be, K.BINS, 3, 4),
    "compaction": lambda be: K.run_compaction(be, K.BINS, 5, "alternating", short=1),
    "predict_rows": lambda be: K.run_predict(be, 1, 1, 1),
    "predict_scene": lambda be: K.run_scene(be, 3, 2, 2, 1),
}


@pytest.mark.parametrize("name", list(POKE_CASES))
def test_a_write_one_element_outside_an_output_is_rejected(name):
    recorder = EmuBackend()
    recorder.forest_launches = trace = []  # forest_kernel_cases.launch appends (kernel, args)
    POKE_CASES[name](recorder)
    pokes = []
    for launch_no, (kernel, args) in enumerate(trace):
        for arg, op in enumerate(args):
            if isinstance(op, K.Op) and op.want.tobytes() != op.init.tobytes():  # an output
                pokes += [(launch_no, arg, elem, kernel, op.name) for elem in outside(op)]
    assert len(pokes) >= 2 * len(trace)
    for launch_no, arg, elem, kernel, op_name in pokes:
        with pytest.raises(AssertionError, match=re.escape(f"{kernel} {op_name}")):
            POKE_CASES[name](Poking(launch_no, arg, elem))
