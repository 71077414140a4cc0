"""TEST INFRASTRUCTURE (no device code): one case per scene-side and classic-ML launch whose grid is capped and finished
by a grid-stride loop -- csrc/components.hip, svm.hip, pairs.hip, match.hip, band_ratio.hip and, of data.hip,
hypel_denorm_scatter, hypel_gather_pairs_f32, hypel_hsi_to_srgb and the two patch launches whose tests stopped short of
their cap -- sized one odd tail past what the capped grid covers in one trip, so that the second trip of the loop runs.

A case names its pass constant (below, each derived from a line of csrc/), counts the work items of its launch at both
sizes -- `big=True`: the smallest size of the issue's shape family that takes a second trip; `big=False`: a few blocks
with the same ragged tail, for the CPU -- and builds its operands, its launch and its expected buffers:

  * every output lives in a buffer pre-filled with a sentinel, GUARD elements longer than the launch may write; the
    expected buffer is that pre-fill with the outputs replaced, so ONE comparison of the whole buffer covers the
    outputs, the pad columns and the sentinels behind them;
  * `late` selects the outputs that only a later trip writes; the CPU test asserts that they differ from the pre-fill,
    so that a tail nobody writes cannot pass;
  * the references are plain vectorised NumPy written for this file (arange arithmetic, shifted-array comparisons,
    sliding_window_view, np.sort, np.repeat), independent of the emulation twins; where the issue names a twin as the
    reference (emu_svm.vote) it is used and a direct count stands beside it.

tests/test_grid_pass_cases_emu.py runs the table at big=False on the emulation, tests/test_gpu_grid_passes.py at
big=True on the device."""
import numpy as np
import torch
from numpy.lib.stride_tricks import sliding_window_view

from hypelcnn_amd.backend import (COLUMN_RANK_WS_WORDS, COMPACT_TILE, COMPONENTS_OK, OUT_DTYPES, SVM_POLY, SVM_RBF, Ref)
from hypelcnn_amd.classic import svc as P
from tests import emu_svm as E

BLOCK = 256          # threads of a block in every launch below (THREADS / SVM_THREADS / block(256))
GRID_CAP = 256 * 8   # csrc/common.h, hypel_grid_1d(work_items, block, max_blocks = 256 * 8)
GUARD = 64           # sentinel elements behind every output

# ---- what one trip of the capped grid covers, by the line of csrc/ that sizes the grid
PASSES = {
    # components.hip flatten / spread_rank / vote / relabel / shadow_correct, pairs.hip pair_masks / points_expand,
    # match.hip add_partials / score / render, svm.hip kernel_apply / kernel_planes / scatter_coef / vote:
    # dim3(hypel_grid_1d(n, THREADS)), one item per thread
    "P": GRID_CAP * BLOCK,
    # svm.hip hypel_svm_vote_score: hypel_grid_1d(rows, SVM_THREADS, 64), one row per thread
    "VOTE_SCORE": 64 * BLOCK,
    # svm.hip hypel_svm_center_norms_f32: hypel_grid_1d(rows, SVM_WAVES), one wave per row, SVM_WAVES = 4 per block
    "CENTER_NORMS": GRID_CAP * (BLOCK // 64),
    # band_ratio.hip hypel_band_ratio_f32: rows_per_block = (THREADS / 64) * (64 >> g_shift), grid = hypel_grid_1d(n,
    # rows_per_block); g_shift = 6 from 33 bands on (a wave per row), 3 at 5..8 bands (eight rows per wave)
    "RATIO_WIDE": GRID_CAP * (BLOCK // 64),
    "RATIO_8": GRID_CAP * (BLOCK // 64) * 8,
    # band_ratio.hip hypel_column_rank_select_f32: per = clamp(ceil(n * col_tiles / 1024), 256, MAX_SLICE = 4096) rows of a
    # block's slice; the items counted here are n * col_tiles
    "HIST_FLOOR": 256 * 1024,
    "HIST_CLAMP": 4096 * 1024,
    # data.hip launch_denorm_scatter: hypel_grid_1d(work, 256, 256 * 64), work in elements or in groups of four bands
    "DENORM": 256 * 64 * BLOCK,
    # data.hip hypel_gather_pairs_f32 / hypel_gather_patches_2x_f32 / hypel_augment_patches_f32: hypel_grid_1d(n, 1,
    # 256 * 32) or (n * p * p, 1, 256 * 32) -- a block per sample row or per patch pixel
    "BLOCK_ITEMS": 256 * 32,
    # data.hip launch_hsi_to_srgb_gv: hypel_grid_1d(n, 256 / G * HSI_PIXELS, 256 * 32) with HSI_PIXELS = 4; G = 16 lanes
    # per group up to 64 lane items, i.e. for the 8-band rasters: 64 pixels per block
    "HSI_G16": 256 * 32 * (BLOCK // 16 * 4),
}
SMALL = 3 * BLOCK    # items of the first "pass" of a big=False case: the tail behind it is the big case's


def pick(big, name, tail):
    """the items of a case whose size is free: one pass and an odd tail"""
    return (PASSES[name] if big else SMALL) + tail


# ===================================================================================================== plumbing
class Expect:
    """want: the whole buffer after the launch; fill: what it held before; late: index (slice, mask, array) of the outputs
    a later trip writes, None where no single output is one; group: late outputs per unit that must differ from the
    pre-fill somewhere (1: every output; a row of converted samples takes every value, the pre-fill's too);
    check(got, want): a comparison other than bytes."""

    def __init__(self, want, fill, late, check=None, group=1):
        self.want, self.fill, self.late, self.check, self.group = want, fill, late, check, group

    def late_outputs_differ(self):
        """(how many units a later trip writes, how many of them look like the pre-fill)"""
        if self.late is None:
            return 0, 0
        late = np.asarray(self.want).reshape(-1)[self.late]
        fill = np.asarray(self.fill, late.dtype)
        differs = (~np.isnan(late) if np.isnan(fill) else late != fill).reshape(-1, self.group).any(axis=1)
        return differs.size, int((~differs).sum())


class Built:
    def __init__(self):
        self.expect = {}     # name -> Expect
        self.facts = []      # (what, bool): properties of the data the case relies on
        self.late_by_fact = False  # no output belongs to a later trip alone: a fact ties the result to the late rows
        self.run = None      # be -> {name: numpy array of the whole buffer}

    def fact(self, what, ok):
        self.facts.append((what, bool(ok)))


def same_bytes(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{name}: {got.dtype}{got.shape} for {want.dtype}{want.shape}"
    a, b = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b) // got.dtype.itemsize
        i = int(bad[0])
        raise AssertionError(f"{name}: {np.unique(bad).size} of {got.size} elements differ; first at {i}: "
                             f"{got.reshape(-1)[i]!r} for {want.reshape(-1)[i]!r}")


def compare(case_name, built, got):
    for name, ex in built.expect.items():
        if ex.check is not None:
            ex.check(f"{case_name} {name}", got[name], ex.want)
        else:
            same_bytes(f"{case_name} {name}", got[name], ex.want)


def padded(values, fill, extra=GUARD):
    """a flat buffer of `values` followed by `extra` sentinels"""
    values = np.asarray(values).reshape(-1)
    out = np.full(values.size + extra, fill, values.dtype)
    out[:values.size] = values
    return out


def sentinel(count, fill, dtype, extra=GUARD):
    return np.full(int(count) + extra, fill, dtype)


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def up16(be, a):
    """uint16 samples travel as int16 bits (torch has no arithmetic on uint16, and none is needed)"""
    a = np.ascontiguousarray(a)
    return be.upload(a.view(np.int16) if a.dtype == np.uint16 else a)


class Case:
    """name; the pass constant; items(big): work items of the capped launch; granule: the step of the shape family (1: the
    size is free and the tail is odd and shorter than a block; None: the shape is that of a sibling case and takes
    several trips with an odd last one; otherwise the big size is the smallest of the family past the pass); twice: the
    launch uses atomics, two runs must give the same bytes; twin: also run on the emulation at the big size (exact
    against the twin)."""

    def __init__(self, name, pass_name, items, build, granule=1, twice=False, twin=False):
        self.name, self.pass_name, self.items, self.build = name, pass_name, items, build
        self.granule, self.twice, self.twin = granule, twice, twin

    def __repr__(self):
        return self.name

    @property
    def pass_items(self):
        return PASSES[self.pass_name]


CASES = []


def case(name, pass_name, items, **kw):
    def register(build):
        CASES.append(Case(name, pass_name, items, build, **kw))
        return build
    return register


# ================================================================================================== components.hip
N_CLASSES, EXCLUDE = 20, (1 << 7) | (1 << 19)
OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def components_shape(big):
    return 9, (58257 if big else 197)   # 9 x 58 257 = 524 313 = P + 25


def rectangles(h, w):
    """mask (y % 4 < 2) & (x % 5 < 3): 2 x 3 rectangles that never touch (the last row and column hold cut ones), their
    root (index of the top-left pixel) and comp (row-major rank of those corners) by arange arithmetic"""
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    mask = (y % 4 < 2) & (x % 5 < 3)
    per_row = (w + 4) // 5
    root = np.where(mask, (y - y % 4) * w + (x - x % 5), -1).astype(np.int32)
    comp = np.where(mask, (y // 4) * per_row + x // 5, -1).astype(np.int32)
    return mask.astype(np.uint8), root, comp, ((h + 3) // 4) * per_row


def shifted(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx]; `fill` outside"""
    h, w = a.shape
    out = np.full_like(a, fill)
    out[max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)] = a[max(0, dy):h - max(0, -dy), max(0, dx):w - max(0, -dx)]
    return out


def component_targets(h, w, mask, seed=3):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, N_CLASSES, (h, w)).astype(np.uint8)
    t[rng.random((h, w)) < 0.25] = 255
    t[:, 40:75] = 255          # components here see no class at all: no winner
    t[:, w - 12:] = 255        # ... and the last of those that only a later trip reaches
    t[mask != 0] = 254         # under the mask: never a vote, kept by relabel where there is no winner
    return t


def vote_reference(targets, comp, n):
    """votes by eight shifted-array comparisons, sizes by a count, winners by strictly-more"""
    t, c = targets.astype(np.int64), comp.astype(np.int64)
    allowed = np.array([k < N_CLASSES and not (EXCLUDE >> k) & 1 for k in range(256)])
    votes = np.zeros((n, N_CLASSES), np.int32)
    for dy, dx in OFFSETS:
        tq, cq = shifted(t, dy, dx, 255), shifted(c, dy, dx, 0)  # outside the image: "in the mask", no vote
        says = (c >= 0) & (cq < 0) & allowed[tq]
        np.add.at(votes, (c[says], tq[says]), 1)
    size = np.bincount(c[c >= 0], minlength=n).astype(np.int32)
    winner = np.where(votes.max(axis=1) > 0, votes.argmax(axis=1), 255).astype(np.uint8)  # argmax: the first maximum
    return votes, size, winner


def pixels(big):
    h, w = components_shape(big)
    return h * w


def first_pass(big, name="P"):
    return PASSES[name] if big else SMALL


@case("components label+compact", "P", pixels, twice=True)
def _(big):
    """flatten_kernel (hypel_components_label_u8) and spread_rank_kernel (hypel_components_compact_i32)"""
    h, w = components_shape(big)
    n = h * w
    mask, root, comp, count = rectangles(h, w)
    late = slice(first_pass(big), n)
    b = Built()
    b.expect["root"] = Expect(padded(root, -7), -7, late)
    b.expect["comp"] = Expect(padded(comp, -7), -7, late)
    b.expect["count"] = Expect(np.array([count, -7], np.int32), -7, slice(0, 1))
    b.expect["status"] = Expect(np.array([COMPONENTS_OK, -7], np.int32), -7, slice(0, 0))
    b.fact("rectangles on both sides of the pass", (root.reshape(-1)[late] >= 0).any() and (root.reshape(-1)[late] < 0).any())
    b.fact("a rectangle straddles a 64-column tile border", mask[0, 191] and mask[0, 192])

    def run(be):
        d_root, d_comp = be.upload(sentinel(n, -7, np.int32)), be.upload(sentinel(n, -7, np.int32))
        d_count, d_status = be.upload(np.array([-7, -7], np.int32)), be.upload(np.array([77, -7], np.int32))
        ws = be.empty(n, torch.int32)
        be.call("components_label_u8", Ref(be.upload(mask)), h, w, Ref(d_root), Ref(ws), Ref(d_status))
        ws2 = be.empty((n + COMPACT_TILE - 1) // COMPACT_TILE, torch.int32)
        be.call("components_compact_i32", Ref(d_root), h, w, Ref(d_comp), Ref(d_count), Ref(ws2))
        be.synchronize()
        return {"root": host(d_root), "comp": host(d_comp), "count": host(d_count), "status": host(d_status)}
    b.run = run
    return b


@case("components votes+relabel", "P", pixels, twice=True)
def _(big):
    """vote_kernel (hypel_components_votes_i32) and relabel_kernel (hypel_components_relabel_u8, plus_one 0 and 1)"""
    h, w = components_shape(big)
    n = h * w
    mask, _, comp, count = rectangles(h, w)
    targets = component_targets(h, w, mask)
    votes, size, winner = vote_reference(targets, comp, count)
    out = np.where((comp >= 0) & (winner[np.maximum(comp, 0)] != 255), winner[np.maximum(comp, 0)], targets).astype(np.uint8)
    out_plus = np.where(out != 255, out + 1, out).astype(np.uint8)
    first = first_pass(big)
    late_px = slice(first, n)
    flat = comp.reshape(-1)
    late_c = np.setdiff1d(flat[first:][flat[first:] >= 0], flat[:first])  # components no pixel of the first trip is in
    b = Built()
    b.expect["votes"] = Expect(padded(votes, -9), -9, None)
    b.expect["size"] = Expect(padded(size, -9), -9, late_c)
    b.expect["winner"] = Expect(padded(winner, 0xAB), 0xAB, late_c)
    b.expect["out"] = Expect(padded(out, 0xAB), 0xAB, late_px)
    b.expect["out_plus_one"] = Expect(padded(out_plus, 0xAB), 0xAB, late_px)
    b.fact("components that only a later trip sees", late_c.size >= 2)
    b.fact("late components with and without a winner", (winner[late_c] == 255).any() and (winner[late_c] != 255).any())
    b.fact("late votes", votes[late_c].sum() > 0)
    b.fact("a tie between two classes decides a winner", ((np.sort(votes, axis=1)[:, -1] == np.sort(votes, axis=1)[:, -2])
                                                        & (votes.max(axis=1) > 0)).any())
    b.fact("relabel paints and keeps late pixels", (out.reshape(-1)[late_px] != targets.reshape(-1)[late_px]).any()
           and (out.reshape(-1)[late_px] == 254).any())

    def run(be):
        d_t, d_comp = be.upload(targets), be.upload(comp)
        d_votes = be.upload(sentinel(count * N_CLASSES, -9, np.int32))
        d_size, d_win = be.upload(sentinel(count, -9, np.int32)), be.upload(sentinel(count, 0xAB, np.uint8))
        be.call("components_votes_i32", Ref(d_t), Ref(d_comp), h, w, count, N_CLASSES, EXCLUDE, Ref(d_votes), Ref(d_size),
                Ref(d_win))
        outs = {}
        for name, plus in (("out", 0), ("out_plus_one", 1)):
            d_out = be.upload(sentinel(n, 0xAB, np.uint8))
            be.call("components_relabel_u8", Ref(d_t), Ref(d_comp), Ref(d_win), h, w, plus, Ref(d_out))
            outs[name] = d_out
        be.synchronize()
        return dict({"votes": host(d_votes), "size": host(d_size), "winner": host(d_win)}, **{k: host(v) for k, v in outs.items()})
    b.run = run
    return b


def correct_shape(big):
    return 3, (58257 if big else 141), 3


def correct_items(big):
    h, w, bands = correct_shape(big)
    return h * w * bands


def correction_case(big, kind):
    from tests.test_components_emu import numpy_correction
    h, w, bands = correct_shape(big)
    rng = np.random.default_rng(17)
    if kind == "uint16 chunky":   # bands 1..3 of a five-band pixel-major raster
        root = rng.integers(0, 60000, (h, w, 5)).astype(np.uint16)
        src, off, strides = root[:, :, 1:4], 1, (w * 5, 5, 1)
    else:                         # bands 1..3 of a four-band band-major raster with three pad columns
        root = (rng.random((4, h, w + 3)) * 3000).astype(np.float32)
        src, off, strides = root[1:4, :, :w].transpose(1, 2, 0), h * (w + 3), (w + 3, 1, h * (w + 3))
    smap = (rng.random((h, w)) < 0.4).astype(np.uint8)
    r_minus_1 = (1 + rng.random(bands) * 4).astype(np.float32) - np.float32(1)
    want = numpy_correction(src, smap, r_minus_1 + np.float32(1))
    n = h * w * bands
    b = Built()
    b.expect["out"] = Expect(padded(want, -7.0), -7.0, slice(first_pass(big), n))
    b.fact("the ratio survives the round trip", np.array_equal((r_minus_1 + np.float32(1)) - np.float32(1), r_minus_1))

    def run(be):
        d_out = be.upload(sentinel(n, -7.0, np.float32))
        be.call("shadow_correct_f32", Ref(up16(be, root), off), OUT_DTYPES[root.dtype], h, w, bands, *strides,
                Ref(be.upload(smap)), Ref(be.upload(r_minus_1)), Ref(d_out))
        be.synchronize()
        return {"out": host(d_out)}
    b.run = run
    return b


for _kind in ("uint16 chunky", "float32 band-major"):
    case(f"shadow_correct {_kind}", "P", correct_items)(lambda big, kind=_kind: correction_case(big, kind))


# ========================================================================================================= svm.hip
TIES = np.float32([-1, 0, 0.0, 1, -0.0, 1e-30, np.nan])   # the tie set of test_vote_bit_exact_on_crafted_ties


@case("svm vote", "P", lambda big: pick(big, "P", 77))
def _(big):
    rows, n_cls, ld = pick(big, "P", 77), 3, 4
    rng = np.random.default_rng(5)
    dec = rng.choice(TIES, size=(rows, ld))
    win = E.vote(dec, n_cls)
    # the same three counts written out: pairs (0,1), (0,2), (1,2); dec > 0 votes for the lower class
    gt = dec[:, :3] > 0
    counts = np.stack([gt[:, 0].astype(int) + gt[:, 1], (~gt[:, 0]).astype(int) + gt[:, 2], (~gt[:, 1]).astype(int) + ~gt[:, 2]], 1)
    labels = np.uint8([10, 20, 30])
    rw = 1031
    rh = (rows + rw - 1) // rw + 1
    where = rng.permutation(rw * rh)[:rows]
    points = np.stack([where % rw, where // rw], axis=1).astype(np.int32)
    raster = np.full(rw * rh, 255, np.uint8)
    raster[where] = labels[win]
    late = slice(first_pass(big), rows)
    b = Built()
    b.expect["out"] = Expect(padded(win.astype(np.uint8), 0xAB), 0xAB, late)
    b.expect["raster"] = Expect(padded(raster, 255), 255, where[late])
    b.fact("the winners are the first maxima of a direct count of dec > 0", np.array_equal(counts.argmax(axis=1), win))
    b.fact("the label counts are those of the direct count", np.array_equal(np.bincount(win, minlength=3),
                                                                           np.bincount(counts.argmax(axis=1), minlength=3)))
    b.fact("every class wins rows of the late trip", np.unique(win[late]).size == 3)

    def run(be):
        d_dec = be.upload(dec)
        d_out, d_raster = be.upload(sentinel(rows, 0xAB, np.uint8)), be.upload(sentinel(rw * rh, 255, np.uint8))
        be.call("svm_vote", Ref(d_dec), ld, rows, n_cls, None, None, Ref(d_out), 0)
        be.call("svm_vote", Ref(d_dec), ld, rows, n_cls, Ref(be.upload(labels)), Ref(be.upload(points)), Ref(d_raster), rw)
        be.synchronize()
        return {"out": host(d_out), "raster": host(d_raster)}
    b.run = run
    return b


@case("svm vote_score", "VOTE_SCORE", lambda big: pick(big, "VOTE_SCORE", 77), twice=True)
def _(big):
    rows, n_cls, n_cells, npp = pick(big, "VOTE_SCORE", 77), 4, 3, 8
    n_pairs = 6
    rng = np.random.default_rng(6)
    dec = rng.choice(TIES, size=(rows, n_cells * npp + 4))
    truth = rng.integers(0, n_cls, rows).astype(np.int32)
    first = first_pass(big, "VOTE_SCORE")
    blocks = [np.ascontiguousarray(dec[:, c * npp:c * npp + n_pairs]) for c in range(n_cells)]
    wins = [E.vote(blk, n_cls) for blk in blocks]
    correct = np.int32([3 + int((w == truth).sum()) for w in wins] + [-9])  # accumulates on what is there
    b = Built()
    b.expect["correct"] = Expect(correct, 3, slice(0, n_cells))
    for c in range(n_cells):
        b.expect[f"labels{c}"] = Expect(padded(wins[c].astype(np.uint8), 0xAB), 0xAB, slice(first, rows))
        b.fact(f"cell {c}: hits in the late trip", (wins[c][first:] == truth[first:]).any())
        b.fact(f"cell {c}: misses", (wins[c] != truth).any())

    def run(be):
        d_dec, d_truth = be.upload(dec), be.upload(truth)
        d_correct = be.upload(np.int32([3] * n_cells + [-9]))
        be.call("svm_vote_score", Ref(d_dec), dec.shape[1], rows, n_cls, n_cells, npp, Ref(d_truth), Ref(d_correct))
        got = {}
        for c in range(n_cells):  # the counts of hypel_svm_vote's labels on the same decisions
            d_lab = be.upload(sentinel(rows, 0xAB, np.uint8))
            be.call("svm_vote", Ref(be.upload(blocks[c])), n_pairs, rows, n_cls, None, None, Ref(d_lab), 0)
            got[f"labels{c}"] = host(d_lab)
        be.synchronize()
        got["correct"] = host(d_correct)
        for c in range(n_cells):
            assert int(got["correct"][c]) == 3 + int((got[f"labels{c}"][:rows] == truth).sum()), f"cell {c}: count != labels"
        return got
    b.run = run
    return b


def center_case(big, ld):
    rows, cols = pick(big, "CENTER_NORMS", 5), 7
    rng = np.random.default_rng(3)
    x = np.full((rows, ld), -7.0, np.float32)
    x[:, :cols] = 2500 + 900 * rng.standard_normal((rows, cols))
    mean = x[:, :cols].astype(np.float64).mean(0).astype(np.float32)
    want = x.copy()
    want[:, :cols] = x[:, :cols] - mean
    ref = (want[:, :cols].astype(np.float64) ** 2).sum(1)
    late = slice(first_pass(big, "CENTER_NORMS"), rows)

    def norms_within(name, got, wanted):  # the bound of test_center_norms_vs_float64
        assert got.shape == wanted.shape and np.array_equal(got[rows:], wanted[rows:]), f"{name}: the sentinels"
        err = np.abs(got[:rows] - wanted[:rows]).max()
        assert err <= 1e-12 * ref.max(), f"{name}: max error {err:.3e} for the bound {1e-12 * ref.max():.3e}"
    b = Built()
    b.expect["x"] = Expect(padded(want, -7.0), -7.0, (np.arange(rows)[late, None] * ld + np.arange(cols)).reshape(-1))
    b.expect["norms"] = Expect(padded(ref, -1.0), -1.0, late, norms_within)
    b.fact("the subtraction changes every value", (want[:, :cols] != x[:, :cols]).all())

    def run(be):
        d_x, d_norms = be.upload(padded(x, -7.0)), be.upload(sentinel(rows, -1.0, np.float64))
        be.call("svm_center_norms_f32", Ref(d_x), ld, rows, cols, Ref(be.upload(mean)), Ref(d_norms))
        be.synchronize()
        return {"x": host(d_x), "norms": host(d_norms)}
    b.run = run
    return b


for _ld, _form in ((8, "float4"), (7, "scalar")):
    case(f"svm center_norms {_form}", "CENTER_NORMS", lambda big: pick(big, "CENTER_NORMS", 5))(
        lambda big, ld=_ld: center_case(big, ld))


def gram_shape(big, vec):
    """rows, cols, ld: 2049 x 1021 with ld = 1024 is 2049 x 256 quads = P + one row of quads; with ld = 1021 the same
    shape goes element by element"""
    rows, cols = (2049, 1021) if big else (41, 77)
    return rows, cols, (cols + 3) // 4 * 4 if vec else cols


def gram_items(vec):
    def items(big):
        rows, cols, ld = gram_shape(big, vec)
        return rows * ((cols + 3) // 4) if vec else rows * cols
    return items


def gram_case(big, vec, seed=9):
    """g = x z^T as float32 in a [rows, ld] buffer whose pad columns hold -7, the float64 norms"""
    rows, cols, ld = gram_shape(big, vec)
    rng = np.random.default_rng(seed)
    x, z = rng.standard_normal((rows, 9)) * 3e3, rng.standard_normal((cols, 9)) * 3e3
    g = np.full((rows, ld), -7.0, np.float32)
    g[:, :cols] = x @ z.T
    return rows, cols, ld, g, (x * x).sum(1), (z * z).sum(1)


def within_2_23(rows, cols, ld):
    """test_kernel_apply_vs_float64's bound on the values, bytes on the pad columns and the sentinels"""
    def check(name, got, want):
        got2, want2 = got[:rows * ld].reshape(rows, ld), want[:rows * ld].reshape(rows, ld)
        err = np.abs(got2[:, :cols].astype(np.float64) - want2[:, :cols]) / np.maximum(np.abs(want2[:, :cols]), 1e-30)
        assert err.max() <= 2.0 ** -23, f"{name}: max relative error {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
        assert np.array_equal(got2[:, cols:], want2[:, cols:].astype(np.float32)), f"{name}: a pad column was written"
        assert np.array_equal(got[rows * ld:], want[rows * ld:].astype(np.float32)), f"{name}: the sentinels"
    return check


def late_values(big, rows, cols, ld):
    """flat positions of the values a later trip writes: quads or elements, in the launch's own item order"""
    first = first_pass(big)
    r, c = np.divmod(np.arange(rows * cols), cols)
    item = r * ((cols + 3) // 4) + c // 4 if ld % 4 == 0 else r * cols + c
    return (r * ld + c)[item >= first]


def apply_case(big, vec, kind):
    rows, cols, ld, g, rn, cn = gram_case(big, vec)
    gamma, coef0, degree = (1e-8, 0.0, 3) if kind == SVM_RBF else (3e-8, 0.5, 3)
    want = g.astype(np.float64)
    want[:, :cols] = E.kernel_values(g[:, :cols], kind, gamma, coef0, degree, rn, cn)  # the float64 evaluation
    b = Built()
    b.expect["g"] = Expect(padded(want, -7.0), -7.0, late_values(big, rows, cols, ld), within_2_23(rows, cols, ld))

    def run(be):
        d_g = be.upload(padded(g, -7.0))
        be.call("svm_kernel_apply_f32", Ref(d_g), ld, rows, cols, kind, gamma, coef0, degree, Ref(be.upload(rn)),
                Ref(be.upload(cn)))
        be.synchronize()
        return {"g": host(d_g)}
    b.run = run
    return b


def planes_case(big, vec):
    rows, cols, ld, g, rn, cn = gram_case(big, vec, seed=10)
    gammas = np.array([1e-8, 3e-8])
    stride = rows * ld + 8
    late = late_values(big, rows, cols, ld)
    b = Built()
    want64 = np.full(2 * stride + GUARD, 7.0)
    for p, gamma in enumerate(gammas):
        v = g.astype(np.float64)
        v[:, :cols] = E.kernel_values(g[:, :cols], SVM_RBF, gamma, 0.0, 3, rn, cn)
        want64[p * stride:p * stride + rows * ld] = v.reshape(-1)

    def planes_ok(name, got, want):
        for p in range(2):
            within_2_23(rows, cols, ld)(f"{name} plane {p}", got[p * stride:(p + 1) * stride], want[p * stride:(p + 1) * stride])
        assert (got[2 * stride:] == 7.0).all(), f"{name}: the sentinels"
    b.expect["planes"] = Expect(want64, 7.0, np.concatenate([late, stride + late]), planes_ok)
    b.expect["g"] = Expect(padded(g, -7.0), -7.0, slice(0, 0))

    def run(be):
        d_g, d_rn, d_cn = be.upload(padded(g, -7.0)), be.upload(rn), be.upload(cn)
        d_out = be.upload(np.full(2 * stride + GUARD, 7.0, np.float32))
        be.call("svm_kernel_planes_f32", Ref(d_g), ld, rows, cols, SVM_RBF, Ref(be.upload(gammas)), 2, Ref(d_rn), Ref(d_cn),
                Ref(d_out), stride)
        be.synchronize()
        planes = host(d_out)
        for p, gamma in enumerate(gammas):  # bit-equal to hypel_svm_kernel_apply_f32 of the same gamma
            d_ref = be.upload(padded(g, -7.0))
            be.call("svm_kernel_apply_f32", Ref(d_ref), ld, rows, cols, SVM_RBF, float(gamma), 0.0, 3, Ref(d_rn), Ref(d_cn))
            ref = host(d_ref)[:rows * ld].reshape(rows, ld)
            got = planes[p * stride:p * stride + rows * ld].reshape(rows, ld)
            same_bytes(f"kernel_planes plane {p} against kernel_apply", got[:, :cols], ref[:, :cols])
            if ld % 4 == 0:
                same_bytes(f"kernel_planes plane {p} against kernel_apply, whole quads", got, ref)
        return {"planes": planes, "g": host(d_g)}
    b.run = run
    return b


for _vec, _form in ((True, "float4"), (False, "scalar")):
    # float4: 2049 rows x 256 quads = 524 544 = P + one row; scalar: the same shape, 2 092 029 elements, four trips
    _kw = dict(granule=256) if _vec else dict(granule=None)
    for _kind, _kname in ((SVM_RBF, "rbf"), (SVM_POLY, "poly3")):
        case(f"svm kernel_apply {_form} {_kname}", "P", gram_items(_vec), **_kw)(
            lambda big, vec=_vec, kind=_kind: apply_case(big, vec, kind))
    case(f"svm kernel_planes {_form}", "P", gram_items(_vec), **_kw)(lambda big, vec=_vec: planes_case(big, vec))


def coef_dims(big):
    return (2049, 16) if big else (33, 3)   # training rows, cells; 2049 x 16 x 16 = 524 544 = P + one row


@case("svm scatter_coef", "P", lambda big: coef_dims(big)[0] * coef_dims(big)[1] * 16, granule=256, twin=True)
def _(big):
    (l, n_c), npp, n_cls = coef_dims(big), 16, 6
    count = np.full(n_cls, l // n_cls, np.int64)
    count[:l % n_cls] += 1
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    tab, total = P.pair_table(start, count)
    n_pairs, n_cols, ldc = len(tab), n_c * npp, n_c * npp + 4
    rng = np.random.default_rng(12)
    alpha_y = rng.standard_normal(n_c * total) * (rng.random(n_c * total) < 0.7)  # zero multipliers too
    rho = rng.standard_normal(n_c * n_pairs)
    dense = np.zeros((l, n_c, npp), np.float32)   # the dense scatter, pair by pair from the table
    for p, rec in enumerate(tab):
        a0, na, b0, nb, off = (int(rec[f]) for f in ("a0", "na", "b0", "nb", "out_off"))
        cell = alpha_y.reshape(n_c, total)[:, off:off + na + nb].astype(np.float32)
        dense[a0:a0 + na, :, p] = cell[:, :na].T
        dense[b0:b0 + nb, :, p] = cell[:, na:].T
    coef = np.full((l, ldc), -7.0, np.float32)
    coef[:, :n_cols] = dense.reshape(l, n_cols)
    bias = np.zeros((n_c, npp), np.float32)
    bias[:, :n_pairs] = (-rho).astype(np.float32).reshape(n_c, n_pairs)
    first = first_pass(big)
    r, c = np.divmod(np.arange(first, l * n_cols), n_cols)
    b = Built()
    b.expect["coef"] = Expect(padded(coef, -7.0), -7.0, r * ldc + c)
    b.expect["bias"] = Expect(padded(bias, -7.0), -7.0, slice(0, 0))
    b.fact("15 pairs and one pad column", n_pairs == 15 and npp - n_pairs == 1 and count.sum() == l)
    b.fact("late coefficients other than zero", (coef.reshape(-1)[r * ldc + c] != 0).any())

    def run(be):
        d_coef, d_bias = be.upload(padded(coef * 0 - 7.0, -7.0)), be.upload(sentinel(n_cols, -7.0, np.float32))
        be.call("svm_scatter_coef_f32", Ref(be.upload(alpha_y)), Ref(be.upload(rho)), Ref(be.upload(tab)), n_pairs, n_c, total,
                l, npp, Ref(d_coef), ldc, Ref(d_bias))
        be.synchronize()
        return {"coef": host(d_coef), "bias": host(d_bias)}
    b.run = run
    return b


# ======================================================================================================= pairs.hip
def masks_case(big, ring):
    n = pick(big, "P", 77)
    rng = np.random.default_rng(21)
    smap = rng.integers(0, 3, n).astype(np.uint8)          # 1: shadow; 0 and 2: not
    reach, margin = (rng.integers(0, 3, n).astype(np.uint8) for _ in range(2))
    lit = smap != 1
    if ring:
        lit = lit & (reach != 0) & (margin == 0)
    late = slice(first_pass(big), n)
    b = Built()
    b.expect["shadow"] = Expect(padded((smap == 1).astype(np.uint8), 9), 9, late)
    b.expect["lit"] = Expect(padded(lit.astype(np.uint8), 9), 9, late)
    b.fact("both values in the late trip", np.unique(lit[late]).size == 2 and np.unique(smap[late] == 1).size == 2)

    def run(be):
        d_sh, d_lit = be.upload(sentinel(n, 9, np.uint8)), be.upload(sentinel(n, 9, np.uint8))
        be.call("pair_masks_u8", Ref(be.upload(smap)), Ref(be.upload(reach)) if ring else None,
                Ref(be.upload(margin)) if ring else None, n, Ref(d_sh), Ref(d_lit))
        be.synchronize()
        return {"shadow": host(d_sh), "lit": host(d_lit)}
    b.run = run
    return b


for _ring in (False, True):
    case("pairs pair_masks" + (" reach+margin" if _ring else ""), "P", lambda big: pick(big, "P", 77))(
        lambda big, ring=_ring: masks_case(big, ring))


def expand_dims(big):
    return (1025, 512, 3) if big else (5, 169, 3)   # 1025 * 512 + 3 = 524 803 = P + one point's repeats + 3


@case("pairs points_expand", "P", lambda big: expand_dims(big)[0] * expand_dims(big)[1] + expand_dims(big)[2], granule=512 + 3)
def _(big):
    n, repeat, remainder = expand_dims(big)
    total = n * repeat + remainder
    rng = np.random.default_rng(22)
    points = rng.integers(0, 2000, (n, 2)).astype(np.int32)
    want = np.vstack([np.repeat(points, repeat, axis=0), points[:remainder]])
    b = Built()
    b.expect["out"] = Expect(padded(want, -7), -7, slice(2 * first_pass(big), 2 * total))

    def run(be):
        d_out = be.upload(sentinel(2 * total, -7, np.int32))
        be.call("points_expand_i32", Ref(be.upload(points)), n, repeat, remainder, Ref(d_out))
        be.synchronize()
        return {"out": host(d_out)}
    b.run = run
    return b


# ======================================================================================================= match.hip
def match_side(big):
    return 730 if big else 33   # a 6 x 6 template: a 725 x 725 = 525 625 surface, the first square one past P (724^2 < P)


def surface_items(big):
    return (match_side(big) - 5) ** 2


def match_case(big, splits, plant):
    """An "int" image (values 0..3: every sum is exact in float32 and in double) with the template itself planted: a
    planted window scores exactly 1, every other one less (Cauchy-Schwarz; the template holds a 1 and a 3, so no window
    of values 0..3 is another multiple of it)."""
    side, ht = match_side(big), 6
    hout = wout = side - ht + 1
    n = hout * wout
    first = first_pass(big)
    rng = np.random.default_rng(31)
    image = rng.integers(0, 4, (side, side)).astype(np.float32)
    tpl = rng.integers(0, 4, (ht, ht)).astype(np.float32)
    tpl[0, 0], tpl[0, 1] = 1, 3
    late_at, early_at = divmod(first + (712 if big else 5), wout), (1, 2)
    spots = {"late": [late_at], "tie": [early_at, late_at]}[plant]
    for y, x in spots:
        image[y:y + ht, x:x + ht] = tpl
    windows = sliding_window_view(image.astype(np.float64), (ht, ht))
    num = np.einsum("yxij,ij->yx", windows, tpl.astype(np.float64))
    energy = np.einsum("yxij,yxij->yx", windows, windows)
    e_t = float((tpl.astype(np.float64) ** 2).sum())
    d = energy * e_t
    with np.errstate(divide="ignore", invalid="ignore"):
        r32 = np.where(d == 0, 0.0, num.astype(np.float32).astype(np.float64) / np.sqrt(d)).astype(np.float32)
    index = int(np.argmax(r32.reshape(-1)))   # the first of equal maxima
    record = np.zeros(16 + GUARD, np.uint8)
    record[16:] = 0xAB
    record[0:4] = np.array([r32.reshape(-1)[index]], np.float32).view(np.uint8)
    record[8:16] = np.array([index], np.int64).view(np.uint8)
    late = slice(first, n)
    b = Built()
    b.expect["num"] = Expect(padded(num.astype(np.float32), -7.0), -7.0, late)
    b.expect["energy"] = Expect(padded(energy, -7.0), -7.0, late)
    b.expect["e_t"] = Expect(np.array([e_t, -7.0]), -7.0, slice(0, 1))
    b.expect["scores"] = Expect(padded(r32, -7.0), -7.0, late)
    b.expect["record"] = Expect(record, 0xAB, slice(0, 0))
    best = np.flatnonzero(r32.reshape(-1) == np.float32(1.0))
    b.fact("the sums are exact in float32", num.max() < 2 ** 24 and np.array_equal(num.astype(np.float32).astype(np.float64), num))
    b.fact("exactly the planted windows score 1", best.tolist() == [y * wout + x for y, x in spots] and r32.max() == 1.0)
    b.fact("the best window is behind the pass, or tied across it",
           best[-1] >= first and (plant == "late" or best[0] < first) and index == best[0])

    def run(be):
        d_img, d_tpl = be.upload(image), be.upload(tpl)
        geo_i, geo_t = (side, side, side, 1, 1), (ht, ht, ht, 1, 1)
        d_num = be.upload(sentinel(n, -7.0, np.float32))
        ws = be.empty(splits * n, torch.float32) if splits > 1 else None
        be.call("match_ccorr_f32", Ref(d_img), *geo_i, Ref(d_tpl), *geo_t, Ref(d_num), None if ws is None else Ref(ws), splits)
        d_energy, d_et = be.upload(sentinel(n, -7.0, np.float64)), be.upload(np.array([-7.0, -7.0]))
        be.call("match_window_energy_f64", Ref(d_img), *geo_i, ht, ht, Ref(d_energy), Ref(be.empty(side * wout, torch.float64)))
        be.call("match_window_energy_f64", Ref(d_tpl), *geo_t, ht, ht, Ref(d_et), Ref(be.empty(ht, torch.float64)))
        d_scores, d_rec = be.upload(sentinel(n, -7.0, np.float32)), be.upload(np.full(16 + GUARD, 0xAB, np.uint8))
        be.call("match_best_f32", Ref(d_num), Ref(d_energy), Ref(d_et), hout, wout, Ref(d_scores), Ref(d_rec))
        be.synchronize()
        return {"num": host(d_num), "energy": host(d_energy), "e_t": host(d_et), "scores": host(d_scores), "record": host(d_rec)}
    b.run = run
    return b


for _splits, _plant in ((2, "tie"), (1, "late")):
    case(f"match score splits={_splits} {_plant}", "P", surface_items, granule=725 ** 2 - 724 ** 2, twice=True)(
        lambda big, splits=_splits, plant=_plant: match_case(big, splits, plant))


def render_side(big):
    return 242 if big else 11   # scale 3: 726 x 726 = 527 076 pixels; 241 * 3 = 723, 723^2 < P


@case("match render", "P", lambda big: (3 * render_side(big)) ** 2, granule=726 ** 2 - 723 ** 2)
def _(big):
    side, scale = render_side(big), 3
    rng = np.random.default_rng(32)
    scene = ((rng.random((side, side, 3)) * 1.2 - 0.2) * 1000).astype(np.float32)   # band 1, read through its strides
    band = scene[:, :, 1]
    top = band.max()
    band[0, 0] = top   # (the maximum itself: grey level 255)
    bigger = np.repeat(np.repeat(band, scale, axis=0), scale, axis=1)
    grey = bigger / top * np.float32(255)
    want = np.clip(grey, 0, 255).astype(np.uint8)
    n = want.size
    b = Built()
    b.expect["out"] = Expect(padded(want, 0xAB), 0xAB, slice(first_pass(big), n))
    b.fact("float32 arithmetic, negative samples and the full level",
           grey.dtype == np.float32 and (band < 0).any() and want.max() == 255)

    def run(be):
        d_out = be.upload(sentinel(n, 0xAB, np.uint8))
        be.call("match_render_u8", Ref(be.upload(scene), 1), side, side, side * 3, 3, scale,
                Ref(be.upload(np.float32([top]))), Ref(d_out))
        be.synchronize()
        return {"out": host(d_out)}
    b.run = run
    return b


# ================================================================================================== band_ratio.hip
def ratio_case(big, pass_name, tail, bands):
    n = pick(big, pass_name, tail)
    first = first_pass(big, pass_name)
    rng = np.random.default_rng(41 + bands)
    ld_num, ld_den, ld_out = bands + 3, bands, bands + 2
    num = (rng.standard_normal((n, ld_num)) * 10.0 ** rng.uniform(-3, 3, (n, ld_num))).astype(np.float32)
    den = (rng.standard_normal((n, ld_den)) * 10.0 ** rng.uniform(-3, 3, (n, ld_den))).astype(np.float32)
    scale = (0.5 + rng.random(bands)).astype(np.float32)
    for i, (row, band) in enumerate(((3, 0), (first - 1, bands - 1), (first, 0), (first + 2, bands // 2), (n - 1, bands - 1))):
        den[row, band] = 0.0                                 # inf, or NaN with a zero numerator
        if i % 2:
            num[row, band] = 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        want = num[:, :bands] / den * scale
    assert want.dtype == np.float32
    ok = np.isfinite(want).all(axis=1)
    ratio = np.full((n, ld_out), -7.0, np.float32)
    ratio[:, :bands] = want
    b = Built()
    b.expect["ratio"] = Expect(padded(ratio, -7.0), -7.0, (np.arange(first, n)[:, None] * ld_out + np.arange(bands)).reshape(-1))
    b.expect["row_ok"] = Expect(padded(ok.astype(np.uint8), 9), 9, slice(first, n))
    b.expect["kept"] = Expect(np.array([ok.sum(), -5], np.int64), -5, slice(0, 1))
    b.fact("dropped rows on both sides of the pass", not ok[first - 1] and not ok[first] and not ok[3] and not ok[n - 1])
    b.fact("kept rows in the late trip", ok[first:].sum() >= 1 and ok.sum() != ok[:first].sum())

    def run(be):
        d_ratio, d_ok = be.upload(sentinel(n * ld_out, -7.0, np.float32)), be.upload(sentinel(n, 9, np.uint8))
        d_kept = be.upload(np.array([-5, -5], np.int64))   # the call clears the count
        be.call("band_ratio_f32", Ref(be.upload(num)), ld_num, Ref(be.upload(den)), ld_den, n, bands, Ref(be.upload(scale)),
                Ref(d_ratio), ld_out, Ref(d_ok), Ref(d_kept))
        be.synchronize()
        return {"ratio": host(d_ratio), "row_ok": host(d_ok), "kept": host(d_kept)}
    b.run = run
    return b


case("band_ratio 65 bands", "RATIO_WIDE", lambda big: pick(big, "RATIO_WIDE", 5), twice=True)(
    lambda big: ratio_case(big, "RATIO_WIDE", 5, 65))
case("band_ratio 7 bands", "RATIO_8", lambda big: pick(big, "RATIO_8", 9), twice=True)(
    lambda big: ratio_case(big, "RATIO_8", 9, 7))


def slice_rows(n, bands):
    """hypel_column_rank_select_f32: the rows of a block's slice"""
    per = (n * ((bands + 31) // 32) + 1023) // 1024
    return (min(max(per, 256), 4096) + 31) // 32 * 32


def select_case(big, n, bands, masked):
    rng = np.random.default_rng(43 + bands)
    x = np.round(rng.standard_normal((n, bands)) * 50, 1).astype(np.float32)   # ties abound
    if bands > 1:
        x[:, 0] = np.float32(-3.25)   # every row of a slice in one bin, at every level
    ok = np.ones(n, np.uint8)
    if masked:
        per = slice_rows(n, bands)
        ok[per:] = rng.random(n - per) >= 0.1   # the first slice whole: the largest count a block can hold
        x[ok == 0] = np.nan                      # a masked row is never read
    x[n - 1, -1], x[n - 2, -1] = -1e6, 1e6       # the extremes of the random column: the last rows of the last slice
    ok[n - 2:] = 1
    kept = int(ok.sum())
    ranks = [0, kept - 1, kept // 2 - 1, kept // 2]
    want = np.sort(x[ok != 0], axis=0)[ranks]
    b = Built()
    b.expect["out"] = Expect(padded(want, np.float32(np.nan)), np.nan, None)
    b.fact("the first and last rank are values of the last slice", want[0, -1] == -1e6 and want[1, -1] == 1e6)
    b.late_by_fact = True
    b.fact("about a tenth of the rows is dropped" if masked else "every row is kept",
           0.85 * n < kept < 0.95 * n if masked and big else kept <= n)

    def run(be):
        d_out = be.upload(sentinel(len(ranks) * bands, np.nan, np.float32))
        ws = be.upload(np.full(bands * COLUMN_RANK_WS_WORDS, 77, np.int32))   # dirty: the call clears it
        be.call("column_rank_select_f32", Ref(be.upload(x)), bands, n, bands, Ref(be.upload(ok)) if masked else None, kept,
                Ref(torch.tensor(ranks, dtype=torch.int64)), len(ranks), Ref(d_out), Ref(ws))
        be.synchronize()
        return {"out": host(d_out)}
    b.run = run
    return b


def floor_rows(big):
    return 262144 + 4097 if big else 1024 + 33     # big: per = ceil(266 241 / 1024) = 261 -> 288 rows, four and a half loops


def clamp_rows(big):
    return 4194304 + 33 if big else 2048 + 33      # big: two bands share a column tile; per = 4097 -> clamped to 4096


case("rank_select slice of 288 rows", "HIST_FLOOR", floor_rows, granule=4097, twice=True)(
    lambda big: select_case(big, floor_rows(big), 1, False))
case("rank_select slice clamped to 4096 rows", "HIST_CLAMP", clamp_rows, twice=True)(
    lambda big: select_case(big, clamp_rows(big), 2, True))


# ======================================================================================================== data.hip
def denorm_case(big, n, bands, ld, dtype, quads):
    from tests.test_gan_inference import EDGES, _cast
    per_row = (bands + 3) // 4 if quads else bands
    first = first_pass(big, "DENORM")
    rng = np.random.default_rng(51 + bands)
    src = (rng.standard_normal((n, ld)) * 1.3).astype(np.float32)
    info = np.iinfo(dtype)
    scale = rng.integers(1, info.max, bands).astype(np.float32)
    offset = rng.integers(0, info.max // 2, bands).astype(np.float32)
    scale[:3], offset[:3] = 1, 0   # the edge values land unscaled in the first bands, in the first and in the last rows
    for rows in (slice(0, 8), slice(n - 8, n)):
        src[rows, :3] = np.resize(EDGES, 24).reshape(8, 3)
    total = n + 5
    perm = rng.permutation(total)[:n].astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        values = _cast((src[:, :bands] * scale) + offset, dtype)
    want = np.full(total * ld * np.dtype(dtype).itemsize, 0xAB, np.uint8).view(dtype).reshape(total, ld).copy()
    fill = want[0, 0]
    want[perm, :bands] = values
    item = np.arange(first, n * per_row)   # the items of the later trips: (row, band) or (row, group of four bands)
    row, j = np.divmod(item, per_row)
    late = (perm[row] * ld + 4 * j)[:, None] + np.arange(4) if quads else (perm[row] * ld + j).reshape(-1, 8)
    b = Built()
    b.expect["out"] = Expect(padded(want, fill), fill, late.reshape(-1), group=late.shape[1])
    b.fact("whole groups of four bands", not quads or bands % 4 == 0)

    def run(be):
        d_out = up16(be, padded(np.full((total, ld), fill, dtype), fill))
        be.call("denorm_scatter", Ref(be.upload(src)), ld, Ref(be.upload(perm)), n, bands, Ref(be.upload(scale)),
                Ref(be.upload(offset)), OUT_DTYPES[np.dtype(dtype)], Ref(d_out), ld)
        be.synchronize()
        return {"out": host(d_out, dtype)}
    b.run = run
    return b


def denorm_scalar_rows(big):
    return 11651 if big else 20           # x 360 bands = 4 194 360 elements: the first row count past the pass


def denorm_quad_rows(big):
    return 1398127 if big else 282        # x 3 quads of 12 bands = 4 194 381 = the pass + 77


case("denorm_scatter scalar uint16", "DENORM", lambda big: denorm_scalar_rows(big) * 360, granule=360)(
    lambda big: denorm_case(big, denorm_scalar_rows(big), 360, 361, np.uint16, False))
case("denorm_scatter float4 uint8", "DENORM", lambda big: denorm_quad_rows(big) * 3)(
    lambda big: denorm_case(big, denorm_quad_rows(big), 12, 12, np.uint8, True))


@case("gather_pairs", "BLOCK_ITEMS", lambda big: pick(big, "BLOCK_ITEMS", 77))
def _(big):
    """gan_train_for_shadow.py's pair gather and its two regulariser swaps, the second one from the swapped spectrum"""
    n, bands, pool, rate = pick(big, "BLOCK_ITEMS", 77), 64, 3000, 0.4
    first = first_pass(big, "BLOCK_ITEMS")
    rng = np.random.default_rng(61)
    normal, shadow = (rng.random((pool, bands)).astype(np.float32) for _ in range(2))
    idx = rng.integers(0, pool, n).astype(np.int64)
    ratio = (1.0 + rng.random(bands)).astype(np.float32)
    u1, u2 = ((rng.random(n) * 0.98 + 0.01).astype(np.float32) for _ in range(2))
    x, y = normal[idx], shadow[idx]
    a, c = u1 < np.float32(rate), u2 < np.float32(rate)
    x = np.where(a[:, None], y * ratio, x)
    y = np.where(c[:, None], x / ratio, y)
    assert x.dtype == np.float32 and y.dtype == np.float32
    late = slice(first * bands, n * bands)
    b = Built()
    b.expect["out_x"] = Expect(padded(x, -7.0), -7.0, late)
    b.expect["out_y"] = Expect(padded(y, -7.0), -7.0, late)
    b.fact("every combination of the two swaps in the late rows", np.unique(2 * a[first:] + c[first:]).size == 4)

    def run(be):
        d_x, d_y = be.upload(sentinel(n * bands, -7.0, np.float32)), be.upload(sentinel(n * bands, -7.0, np.float32))
        be.call("gather_pairs_f32", Ref(be.upload(normal)), Ref(be.upload(shadow)), Ref(be.upload(idx)), n, bands,
                Ref(be.upload(ratio)), Ref(be.upload(u1)), Ref(be.upload(u2)), rate, Ref(d_x), Ref(d_y))
        be.synchronize()
        return {"out_x": host(d_x), "out_y": host(d_y)}
    b.run = run
    return b


@case("hsi_to_srgb 8 bands uint8", "HSI_G16", lambda big: pick(big, "HSI_G16", 77))
def _(big):
    """the byte rendering of an 8-band uint8 raster (tight rows: four bands per lane, 16 lanes per group) against the
    float64 oracle of tests/rgb_cases.py under its pass rule"""
    from hypelcnn_amd.backend import RGB_U8
    from hypelcnn_amd.common import hsi_rgb_converter as HR
    from tests import rgb_cases as RC
    n, bands = pick(big, "HSI_G16", 77), 8
    first = first_pass(big, "HSI_G16")
    rng = np.random.default_rng(62)
    bm = RC.measurements(bands)
    lo, hi = RC.normalisation(np.uint8, bands, True, rng)
    raster = np.roll(RC.edge_raster(1, n, bands, bands, np.uint8, lo, hi, rng), n - 50, axis=0)  # the edge rows: in the late trip
    want = RC.oracle_u8(bm, raster[:, :bands], lo, hi)
    band0, span, table = HR.render_table(bm, bands, hi, lo)

    def within_the_pass_rule(name, got, wanted):
        assert (got[3 * n:] == 0xAB).all(), f"{name}: the sentinels"
        RC.check_u8(got[:3 * n].reshape(n, 3), wanted[:3 * n].reshape(n, 3))
    b = Built()
    b.expect["rgb"] = Expect(padded(want, 0xAB), 0xAB, slice(3 * first, 3 * n), within_the_pass_rule, group=3)
    b.fact("four bands per lane, 16 lanes per group", ((span + 3) // 4 + 3) // 4 <= 16 and raster.shape[1] % 4 == 0)
    b.fact("black, white and colours in the late trip", {0, 255} <= set(want[first:].reshape(-1).tolist())
           and (want[first:].std(axis=1) > 0).any())

    def run(be):
        d_out = be.upload(sentinel(3 * n, 0xAB, np.uint8))
        be.call("hsi_to_srgb", Ref(be.upload(raster)), OUT_DTYPES[np.dtype(np.uint8)], bands, n, bands, band0, span,
                Ref(be.upload(table)), Ref(be.upload(HR.srgb_levels())), RGB_U8, Ref(d_out))
        be.synchronize()
        return {"rgb": host(d_out)}
    b.run = run
    return b


# hypel_gather_patches_2x_f32 and hypel_augment_patches_f32 walk a block per patch pixel: the runners of
# tests/head_kernel_cases.py (NumPy slicing / the torch composition as references, sentinel windows) at 911 patches of
# 3 x 3 pixels, 8199 = BLOCK_ITEMS + 7 items
GATHER_2X_WALK = dict(nb=1, cc=94, cl=2, n=911, h=30, w=31)
AUGMENT_WALK = dict(c=96, n=911, p=3, selectors=("rot_k", "ratio", "flip_lr", "flip_ud", "delta"), with_idx=True)


def by_name(name):
    return next(c for c in CASES if c.name == name)
