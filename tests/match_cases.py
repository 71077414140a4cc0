"""TEST INFRASTRUCTURE: the template-matching cases and their float64 reference -- a NumPy restatement of DESIGN §3.12
(cv2.resize INTER_AREA by an integer factor = pixel replication, cv2.matchTemplate TM_CCORR_NORMED, cv2.minMaxLoc's
max_loc), shared by the CPU tests of the emulation and the GPU tests of csrc/match.hip.  The replication is materialised
with numpy.repeat and the windows are taken through sliding_window_view, neither of which the kernels or their
emulation do.

Every case exists in two kinds: "int" (values 0..3: every sum is exact in float32 and in double, so everything is
compared bit for bit) and "uniform" (values in [-1, 1]: compared within the bounds below).  The shapes are the smallest at
which the launches can still go wrong; the chunk case is sized from the library's constants."""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from hypelcnn_amd.backend import MATCH_BLOCK_COLS, MATCH_COL_CHUNK, MATCH_ROW_CHUNK, MATCH_TILE

U24, U53 = 2.0 ** -24, 2.0 ** -53


def _plain(h, w):
    return lambda fill: fill((h, w))


def _band(h, w, bands, b):
    return lambda fill: fill((h, w, bands))[:, :, b]  # a view: read in place through its strides


def _band_transposed(h, w, bands, b):
    return lambda fill: fill((w, h, bands))[:, :, b].T  # a band of a [w][h][bands] store: sx = h * bands > sy = bands


def _zero_block(h, w, rows, cols):
    def make(fill):
        a = fill((h, w))
        a[rows, cols] = 0
        return a
    return make


def _all_zero(h, w):
    def make(fill):
        return fill((h, w)) * 0 if fill.kind == "int" else fill((h, w))  # uniform: the shape only
    return make


def _signed(h, w, positive=None):
    """uniform kind only: magnitudes as drawn, every sign negative but the one at `positive` (None: all positive).  A
    1 x 1 template scores exactly +-1 everywhere, so its uniform case has a unique best only if one pixel alone agrees
    in sign with the template."""
    def make(fill):
        a = fill((h, w))
        if fill.kind == "int":
            return a
        a = np.maximum(np.abs(a), np.float32(2.0 ** -10))
        if positive is not None:
            a = -a
            a[positive] = -a[positive]
        return a
    return make


def _periodic(h, w, py, px):
    def make(fill):
        if fill.kind != "int":
            return fill((h, w))  # uniform: the shape only (identical windows cannot have a unique best)
        return np.ascontiguousarray(np.tile(fill((py, px)), (h // py + 1, w // px + 1))[:h, :w])
    return make


# name -> (image maker, image scale, template maker, template scale)
CASES = {
    "whole_image_7x9": (_plain(7, 9), 1, _plain(7, 9), 1),
    "template_1x1": (_signed(7, 9, positive=(4, 6)), 1, _signed(1, 1), 1),
    "full_height": (_plain(9, 20), 1, _plain(9, 5), 1),
    "full_width": (_plain(20, 9), 1, _plain(5, 9), 1),
    # a template one past the staged chunk in both axes; three tiles per axis with a ragged last one
    "chunks_plus_one": (_plain(2 * MATCH_TILE + 4 + MATCH_ROW_CHUNK, 2 * MATCH_TILE + 10 + MATCH_COL_CHUNK), 1,
                        _plain(MATCH_ROW_CHUNK + 1, MATCH_COL_CHUNK + 1), 1),
    # more than one block across, the last one with a single active wave and a ragged sub-tile
    "blocks_across": (_plain(8, MATCH_BLOCK_COLS + 40 + 6), 1, _plain(4, 7), 1),
    "scales_5_2": (_plain(13, 17), 5, _plain(9, 11), 2),
    "scales_1_3": (_plain(29, 37), 1, _plain(9, 11), 3),
    "scales_4_1": (_plain(13, 17), 4, _plain(9, 11), 1),
    "strided_bands": (_band(20, 24, 5, 3), 1, _band(6, 7, 3, 2), 1),
    "strided_bands_scaled": (_band(10, 12, 5, 3), 3, _band(6, 7, 3, 2), 2),
    "transposed_band": (_band_transposed(29, 37, 5, 3), 1, _band_transposed(9, 11, 3, 2), 3),
    "zero_block": (_zero_block(20, 24, slice(3, 13), slice(5, 17)), 1, _plain(4, 5), 1),
    "all_zero_image": (_all_zero(12, 15), 1, _plain(4, 5), 1),
    "ties_periodic": (_periodic(14, 19, 3, 4), 1, _plain(5, 6), 1),
}
KINDS = ("int", "uniform")
# uniform kind: seeds chosen on the CPU so that the reference's best score beats every other one by more than twice
# the bound on R (test_match_emu.test_uniform_cases_have_a_clear_winner asserts it for every case)
SEEDS = {name: 0 for name in CASES}


class _Fill:
    def __init__(self, kind, rng):
        self.kind, self.rng = kind, rng

    def __call__(self, shape):
        if self.kind == "int":
            return self.rng.integers(0, 4, shape).astype(np.float32)
        return self.rng.uniform(-1, 1, shape).astype(np.float32)


def replicate(a, scale):
    return np.repeat(np.repeat(a, scale, axis=0), scale, axis=1)


class Case:
    """image / template: float32 2-D arrays (possibly strided views) and their scales; the float64 reference: num,
    abs_num (sum |T'| |I'|), energy, e_t, r (float64), r32 (the float32 surface) and index (first maximum of r32)."""

    def __init__(self, name, kind):
        make_image, self.image_scale, make_template, self.template_scale = CASES[name]
        rng = np.random.default_rng([SEEDS[name], KINDS.index(kind)] + [ord(c) for c in name])
        fill = _Fill(kind, rng)
        self.name, self.kind = name, kind
        self.image, self.template = make_image(fill), make_template(fill)
        big = replicate(self.image.astype(np.float64), self.image_scale)
        tpl = replicate(self.template.astype(np.float64), self.template_scale)
        self.H, self.W = big.shape
        self.ht, self.wt = tpl.shape
        self.hout, self.wout = self.H - self.ht + 1, self.W - self.wt + 1
        windows = sliding_window_view(big, tpl.shape)
        self.num = np.einsum("yxij,ij->yx", windows, tpl)
        self.abs_num = np.einsum("yxij,ij->yx", np.abs(windows), np.abs(tpl))
        self.energy = np.einsum("yxij,yxij->yx", windows, windows)
        self.image_energy = float((big * big).sum())
        self.e_t = float((tpl * tpl).sum())
        d = self.energy * self.e_t
        with np.errstate(divide="ignore", invalid="ignore"):
            self.r = np.where(d == 0, 0.0, self.num / np.sqrt(d))
            # the surface the launches define: the float32 numerator over the double energies
            self.r32 = np.where(d == 0, 0.0, self.num.astype(np.float32).astype(np.float64) / np.sqrt(d)).astype(np.float32)
        self.index = int(np.argmax(self.r32.reshape(-1)))
        n = self.ht * self.wt
        self.num_bound = (n + 8) * U24 * self.abs_num
        self.energy_bound = 4 * self.H * self.W * U53 * self.image_energy
        self.r_bound = (n + 16) * U24

    def clear_winner(self):
        """the reference's best score beats every other one by more than twice the bound on R"""
        flat = np.sort(self.r.reshape(-1))
        return flat.size == 1 or flat[-1] - flat[-2] > 2 * self.r_bound


@functools.lru_cache(maxsize=None)
def case(name, kind):
    return Case(name, kind)
