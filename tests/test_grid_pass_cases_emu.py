"""CPU: the grid-pass cases of tests/grid_pass_cases.py.  Every case at its reduced size on the emulation against the
case's own NumPy reference; the size of every case on the device -- past its pass constant, by an odd tail shorter than a
block where the size is free, by the smallest step of its shape family otherwise; and the outputs that only a later trip
of the grid-stride loop writes differ from what the buffer held before, so that a tail nobody writes cannot pass."""
import pytest

import tests.emu_band_ratio  # noqa: F401 -- the launches register on EmuBackend
import tests.emu_components  # noqa: F401
import tests.emu_match  # noqa: F401
import tests.emu_pairs  # noqa: F401
import tests.emu_svm  # noqa: F401
import tests.emu_svm_grid  # noqa: F401
from tests import grid_pass_cases as G
from tests import head_kernel_cases as H
from tests import parity_util as PU
from tests.rgb_cases import RgbEmu  # EmuBackend + the specifications of hypel_denorm_scatter and hypel_hsi_to_srgb


def test_the_pass_constants_are_the_launch_code_s():
    """the lines the constants are derived from still read that way"""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hypelcnn_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("common.h", "svm.hip", "band_ratio.hip", "data.hip")}
    assert "int max_blocks = 256 * 8" in text["common.h"]
    assert "hypel_grid_1d(rows, SVM_THREADS, 64)" in text["svm.hip"] and "hypel_grid_1d(rows, SVM_WAVES)" in text["svm.hip"]
    assert "constexpr int SVM_THREADS = 256;" in text["svm.hip"]
    assert "(int64_t)(THREADS / 64) * (64 >> g_shift)" in text["band_ratio.hip"]
    assert "per < 256 ? 256 : per > MAX_SLICE ? MAX_SLICE : per" in text["band_ratio.hip"]
    assert "(n * col_tiles + 1023) / 1024" in text["band_ratio.hip"] and "MAX_SLICE = 4096" in text["band_ratio.hip"]
    assert "hypel_grid_1d(work, 256, 256 * 64)" in text["data.hip"]
    assert G.slice_rows(G.floor_rows(True), 1) == 288 and G.slice_rows(G.clamp_rows(True), 2) == 4096
    assert G.slice_rows(G.floor_rows(True) - 4097, 1) == 256 and G.slice_rows(G.clamp_rows(True) - 33, 2) == 4096


@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_big_size_is_one_odd_tail_past_the_pass(case):
    items, one_pass = case.items(True), case.pass_items
    tail = items - one_pass
    assert tail > 0, "no second trip"
    if case.granule == 1:        # a free size: less than a block's worth, ragged (no whole wave) and odd
        assert tail < G.BLOCK and tail % 64 != 0 and tail % 2 == 1, tail
    elif case.granule is None:   # the shape of its float4 sibling: several trips, the last one ragged and odd
        last = items % one_pass
        assert items > one_pass and last % G.BLOCK != 0 and last % 2 == 1, last
    else:                        # the smallest size of its shape family that takes the second trip
        assert items - case.granule <= one_pass, (items, case.granule)
        assert tail % 64 != 0 or tail <= G.BLOCK, tail
    small = case.items(False)
    assert G.SMALL < small < items and (small - G.SMALL) % 64 != 0   # the reduced size: more than one block, a ragged tail


@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_reduced_case_on_the_emulation(case):
    built = case.build(False)
    for what, ok in built.facts:
        assert ok, f"{case.name}: {what}"
    written = 0
    for name, ex in built.expect.items():
        units, like_fill = ex.late_outputs_differ()
        written += units
        assert like_fill == 0, f"{case.name} {name}: {like_fill} of {units} late outputs equal the pre-fill {ex.fill!r}"
    assert written > 0 or built.late_by_fact, f"{case.name}: no output is known to come from a later trip"
    got = built.run(RgbEmu())
    G.compare(case.name, built, got)


def test_patch_walks_on_the_specification():
    """the two launches with a block per patch pixel, through the runners of tests/head_kernel_cases.py"""
    for walk in (G.GATHER_2X_WALK, G.AUGMENT_WALK):
        tail = walk["n"] * 9 - G.PASSES["BLOCK_ITEMS"]
        assert 0 < tail < G.BLOCK and tail % 2 == 1
    assert G.GATHER_2X_WALK["h"] * G.GATHER_2X_WALK["w"] >= G.GATHER_2X_WALK["n"] and 2 * G.GATHER_2X_WALK["nb"] + 1 == 3
    H.run_gather_2x(PU.SpecOnly(), **G.GATHER_2X_WALK)
    H.run_augment(PU.SpecOnly(), **G.AUGMENT_WALK)
