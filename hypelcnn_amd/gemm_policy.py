"""How one grouped GEMM product becomes launches: split-K, the tile-width hint, fp32 versus split-operand kernels,
K-slice records chosen by a simulated schedule, the filter-gradient row / pixel splits.  Pure functions of `GemmTables`,
a `GemmShape` and a few integers -- no tower, session or backend -- with the tunables each one reads in front of it.

A tunable has ONE home: readers elsewhere go through this module (`gemm_policy.KSLICE_MIN_K`), never through a
`from ... import` copy, so that a test's monkeypatch.setattr and HYPEL_PLAN_SET (plan.py) reach every reader.  The flag
bits and the tile height of the ABI are read through gemm_tables (`T.GEMM_VAR_N`, `T.GEMM_BM`) for the same reason."""
import heapq
import os

from . import gemm_tables as T

SPLITK_BELOW = 400    # FC-shaped products with fewer 128x64 blocks are cut along K
SPLITK_TARGET = 768  # ... into slices that give about this many blocks
GEMM_BK = 32  # reduction columns per k-tile of the fp32 kernels


def cut_segments(gs, s_, a_ks, b_ks, grain=16):
    """Cut a segment list into s_ slices of (nearly) equal reduction length, at multiples of `grain` columns of the
    whole list (16: the split kernels' k-tile; GEMM_BK: the fp32 kernels'); a_ks / b_ks = element distance of one
    reduction column in A / B."""
    ktot = sum(k for _, _, k in gs)
    cuts = [min(ktot, (ktot * i // s_ + grain - 1) // grain * grain) for i in range(s_)] + [ktot]
    parts = [[] for _ in range(s_)]
    base = 0
    for (a_off, b_off, k) in gs:
        for i in range(s_):
            lo, hi = max(cuts[i], base), min(cuts[i + 1], base + k)
            if hi > lo:
                parts[i].append((a_off + (lo - base) * a_ks, b_off + (lo - base) * b_ks, hi - lo))
        base += k
    return parts


def split_k(tables, shape):
    """FC-shaped products have too few 128x128 output tiles to fill 256 CUs (fc_0 forward: 64 blocks;
    image_gen_net_4 data gradient: 32).  When the output is one dense range, cut every group's K into S
    slices that write partial slabs; hypel_reduce_splits_f32 sums them in a fixed order.
    Returns None or (the sliced tables, S, first output element, elements of one slab)."""
    groups, n = tables.groups, shape.n
    if shape.ldc != n or not groups:
        return None
    n_nt = (n + 63) // 64 if n > 32 else 1
    blocks = sum((rows + T.GEMM_BM - 1) // T.GEMM_BM for _, _, rows in groups) * n_nt
    kmax = max(tables.ksum(gi) for gi in range(len(groups)))
    if blocks >= SPLITK_BELOW or kmax < 512:
        return None
    S = min((SPLITK_TARGET + blocks - 1) // blocks, kmax // 128, 32)
    if S < 2:
        return None
    order = sorted(groups, key=lambda g: g[0])
    c_min = order[0][0]
    pos = c_min
    for c_off, _, rows in order:  # dense, gap-free cover
        if c_off != pos:
            return None
        pos += rows * n
    count = pos - c_min
    if c_min % n:
        return None
    out = T.GemmTables()
    for c_off, gs, rows in groups:
        for s, part in enumerate(cut_segments(gs, S, shape.a_ks, shape.b_ks, grain=GEMM_BK)):
            out.add_group(s * count + (c_off - c_min), part, rows)
    return out, S, c_min, count


# per-launch A/B: HYPEL_HINT_OVERRIDE="fwd:conv_enc_2=1,dgrad:fc_0=2"
HINT_OVERRIDE = {k: int(v) for k, v in (kv.split("=") for kv in os.environ.get("HYPEL_HINT_OVERRIDE", "").split(",") if kv)}
RESIDENT_BLOCKS_64 = 6 * 256  # 128x64 (and multi-segment 128x32) blocks the device holds at once


def tile_hint(tables, shape, folded):
    """Tile-width hint for hypel_seg_gemm_f32 (bits 8-9 of `accumulate`), from the per-launch A/B measurements in
    profiles/r1_gemm_tile_choice*.txt (HYPELCNN at N=1024 and DUALCNN at N=512): 1 = 128x32, 2 = 128x64.
    Wide tiles win whenever a launch has plenty of blocks; narrow ones balance small launches, and the data
    gradients that also gather the shortcut gradient in their epilogue (more, shorter epilogues overlap better)."""
    n, ta, tb = shape.n, shape.ta, shape.tb
    if n <= 32:
        return 0
    n_tiles = sum((rows + T.GEMM_BM - 1) // T.GEMM_BM for _, _, rows in tables.groups)
    blocks64 = n_tiles * ((n + 63) // 64)
    if tb and not ta:
        ks = [k for _, segs, _ in tables.groups for _, _, k in segs]
        if ks and sum(ks) / len(ks) < 48:
            # short segments: per-k-tile overhead dominates, keep the wide tile -- unless that leaves the launch
            # with under ~1000 blocks (the n = 120 data gradient of the 15-filter level: 142 us on 128x32 tiles,
            # 154 on 128x64, round-2 A/B with paired segments)
            if blocks64 < 1000:
                return 1
            # ... and unless the 64-wide tiling overflows the resident capacity (6 blocks per CU) by a few blocks: the
            # level-1 data gradient of H13 (392 x 4 = 1568 on 1536) then ends in a round of 32 lone blocks, and the
            # 32-wide tiling (3136 blocks, two even rounds) is 46 us faster per step
            over = blocks64 % RESIDENT_BLOCKS_64
            return 1 if blocks64 < 2 * RESIDENT_BLOCKS_64 and 0 < over <= RESIDENT_BLOCKS_64 // 10 else 2
        if folded and blocks64 < 4000:
            return 1
        return 1 if blocks64 < 900 else 2
    if ta:
        return 1 if blocks64 < 900 else 2
    # forward.  Round-2 per-launch A/B of the three tile widths (tools/gemm_microbench.py, HYPEL_GEMM_FORCE_WIDTH):
    # single-segment products (1x1 convolutions, n <= 512) run fastest on 128x32 tiles -- except n = 480, which
    # tiles 5 x 96 without padding and whose 392 x 5 blocks are just under two resident rounds of the 128x96
    # variant (conv_dec_0 218 vs 227 (32) vs 244 (64) us; conv_enc_2 129 vs 134 vs 138) -- multi-segment levels
    # and the very wide dense layers on 128x64.
    if n <= 512 and all(len(segs) == 1 for _, segs, _ in tables.groups):
        if n >= 480 and n % 96 == 0:
            return 3
        return 1
    return 1 if blocks64 < 768 else 2


# fp32 products on the bf16 matrix cores with three-way split operands and six partial products (include/hypel.h
# HYPEL_GEMM_SPLIT6): "0" = never, "6" = wherever the launch is eligible and large enough (widths by column count),
# "6:W" = the same with the tile width forced to hint W (1 = 128x32, 2 = 128x64, 3 = 128x128; per-launch A/B).
# HYPEL_SPLIT_OVERRIDE="fwd:conv_dec_0=3,dgrad:conv_dec_0=0": per launch tag, 0 = fp32 MFMA kernel.
_gs = os.environ.get("HYPEL_GEMM_SPLIT", "6").split(":")
GEMM_SPLIT = int(_gs[0] or 0)
GEMM_SPLIT_WIDTH = int(_gs[1]) if len(_gs) > 1 else 0
GEMM_SPLIT_MIN_FLOPS = float(os.environ.get("HYPEL_GEMM_SPLIT_MIN_GFLOP", "2")) * 1e9  # ... of the launch at SPLIT_NOMINAL_BATCH samples
SPLIT_NOMINAL_BATCH = 1024  # batch the size rule prices a classifier launch at (the kernel family is chosen per layer, not per batch)
SPLIT_NOMINAL_BATCH_GAN = 4096  # ... and a GAN train op's (PhasePlan: the pair batch of BASELINE's CUT configuration)
# narrow products stage a whole 128-row A tile per 32 output columns: the split costs more than the matrix rate returns
# (H13 level 1, 30 filters per branch: 382 -> 397 us forward, 103 -> 95 TFLOP/s filter gradient; per-launch A/B, round 5)
GEMM_SPLIT_MIN_N = 32
SPLIT_OVERRIDE = {k: int(v) for k, v in (kv.split("=") for kv in os.environ.get("HYPEL_SPLIT_OVERRIDE", "").split(",") if kv)}
SPLIT6_BN = {1: 32, 2: 64, 3: 128}  # output columns of the split kernels' blocks, by tile-width hint


def split6_width(n):
    """Tile-width hint of a split-operand launch by its column count: 128x128 blocks unless the last column tile
    would be more than half empty."""
    if GEMM_SPLIT_WIDTH:
        return GEMM_SPLIT_WIDTH
    if n <= 32:
        return 1
    rem = n % 128
    return 2 if n <= 64 or 0 < rem <= 64 and n < 256 else 3


def split6(tag, tables, shape, flags, paired, nb, nominal_batch, in_multi=False):
    """0 = fp32 MFMA kernel, else the tile-width hint of the split-operand kernel for this launch.  in_multi: a product
    of the merged filter-gradient launch -- it shares its launch with the other products of its width class, so its
    own size does not matter (left on the fp32 kernels, the few small ones formed a 102 us launch of 4.4 GFLOP).
    The choice is a function of the LAYER, not of the batch: the size rule prices the launch (of nb samples) at
    nominal_batch samples (every product of the path is linear in the batch), so that a sample meets the same arithmetic
    at batch 64, 512 and 1024 and on 1 or 8 ranks (round-5 verdict: the FLOP count of the launch itself made it
    batch-dependent)."""
    n, ta, tb = shape.n, shape.ta, shape.tb
    eligible = n > 16 and not (ta and tb) and not (flags & ~T.GEMM_VAR_N) and not paired
    if tag in SPLIT_OVERRIDE:
        w = SPLIT_OVERRIDE[tag]
        if w and not eligible:
            raise ValueError(f"HYPEL_SPLIT_OVERRIDE: launch {tag!r} (n = {n}, trans = {int(bool(ta))}{int(bool(tb))}, "
                             f"flags = {flags:#x}, paired segments = {bool(paired)}) cannot run on the split-operand "
                             "kernels (they need n > 16, a plain NN / NT / TN product, no 16x16x4 / activation epilogue)")
        if w not in (0, 1, 2, 3):
            raise ValueError(f"HYPEL_SPLIT_OVERRIDE: width hint {w} for {tag!r} (0 = fp32 kernel, 1 / 2 / 3 = 128x32 / x64 / x128)")
        return w
    if GEMM_SPLIT != 6 or n <= GEMM_SPLIT_MIN_N or not eligible:
        return 0
    if in_multi:
        return split6_width(n)
    macs = sum(rows * tables.ksum(gi) * tables.n_of(gi, n) for gi, (_, _, rows) in enumerate(tables.groups))
    if 2 * macs * nominal_batch < GEMM_SPLIT_MIN_FLOPS * nb:
        return 0
    return split6_width(n)


def col_tiles(n, sp6=0):
    """[(n0, tile width)] of a product of the merged filter-gradient launch with n output columns: one width per
    product.  sp6 = tile-width hint of the split-operand kernel (widths | GEMM_MULTI_SPLIT6: their own launches)."""
    if sp6:
        wdt = SPLIT6_BN[sp6]
        return [(n0, wdt | T.GEMM_MULTI_SPLIT6) for n0 in range(0, n, wdt)]
    wdt = 16 if n <= 16 else (32 if n <= 32 else 64)
    return [(n0, wdt) for n0 in range(0, n, wdt)]


# K-slice records for the split-operand kernels (include/hypel.h HYPEL_TILE_PLAIN; round-5 verdict item 1).  The 128-wide
# split blocks have 512 resident slots (two per CU), a third of what the fp32 kernels had: a data gradient of 392 x 4 = 1 568
# equal blocks runs 3.06 rounds and pays for 4, and the 392 blocks of a multi-kernel level's data gradient are all resident
# at once and the launch lasts as long as its heaviest tile (the centre pixel sums 1.57x the mean).  The planner SIMULATES the
# launch -- list scheduling of the blocks in table order on 64 slots per XCD -- for a few slicings (every tile above a K
# threshold cut into equal slices; the tiles of each XCD's last, partly filled round cut into s slices) and takes the best
# one if it beats the unsliced launch by KSLICE_MIN_GAIN.  Slices >= 1 write plain partials to scratch, one
# hypel_reduce_splits_multi_sized_f32 adds them in slice order.
KSLICE_MIN_GAIN = 0.10
KSLICE_OVERHEAD_K = 24   # fixed cost of a block in reduction columns (prologue, pipeline fill, epilogue)
KSLICE_MIN_K = 48        # shortest slice (reduction columns)
KSLICE_MAX_SLICES = 16
KSLICE_FRAC_MIN = 0.7    # smallest threshold (fraction of the launch's heaviest tile) above which tiles are sliced.  Same box
#                          (profiles/r6_exp_kslice.txt), the 60-filter level's data gradient, 392 tiles: unsliced 319 us; threshold
#                          0.7 (496 records) 279 us; 0.5 (688: a second round) 299; 0.25 (960) 267 -- but with three times the
#                          partial traffic; the simulation, which knows nothing of two blocks sharing a CU, prefers 0.25
KSLICE_REDUCE_COST_K = 55  # the reduce launch behind a sliced launch (~6 us), in reduction columns of a 128 x 128 block
KSLICE_SLOTS = {1: 768, 2: 512, 3: 512}  # resident blocks of the split kernels by tile-width hint (3 / 2 / 2 per CU)


def kslice_makespan(shares, extra, slots):
    """Simulated duration of a launch laid out as GemmTables.finalize lays it out: shares = eight lists of block costs in
    dispatch order, extra = block costs dealt heaviest first to the end of the least loaded share; every XCD runs its list
    on slots / 8 block slots, next block to the slot that frees first."""
    dealt, _ = T.xcd_deal(extra, lambda c: c, [sum(sh) for sh in shares])
    per = max(1, slots // T.XCDS)
    worst = 0.0
    for sh, d in zip(shares, dealt):
        free = [0.0] * per
        for c in list(sh) + d:
            t = heapq.heappop(free)
            heapq.heappush(free, t + c)
        worst = max(worst, max(free))
    return worst


def kslice(tables, shape, width_hint):
    """Choose K-slices for a launch on the split kernels (see KSLICE_MIN_GAIN above).  Returns None (leave the launch
    alone) or {group index: number of slices}."""
    groups = tables.groups
    bn = SPLIT6_BN[width_hint]
    slots = KSLICE_SLOTS[width_hint]
    ct = (shape.n + bn - 1) // bn
    ov = KSLICE_OVERHEAD_K
    ksums = [tables.ksum(gi) for gi in range(len(groups))]
    order = [(gi, ksums[gi]) for _, gi, _, _ in tables.tile_order()]  # (group, its K) per tile record, in dispatch order

    def evaluate(slices):  # slices: {gi: s}
        main = [t for t in order if slices.get(t[0], 1) == 1]
        extra, pieces = [], 0
        for gi, ksum in order:
            s_ = slices.get(gi, 1)
            if s_ > 1:
                extra += [ksum / s_ + ov] * (s_ * ct)
                pieces += (s_ - 1) * ct
        sh = [[ksum + ov for _, ksum in share for _ in range(ct)] for share in T.xcd_shares(main)]
        # + what the partials cost: a 128 x bn partial is written, read back and added into the output (~3 passes of
        # 512 bn bytes at ~4 TB/s; one reduction column of a 128 x 128 block is ~0.11 us), + the reduce launch (~6 us)
        traffic = pieces * (3 * 512 * bn / 4e12) / (0.11e-6 * bn / 128)
        return kslice_makespan(sh, extra, slots) + (traffic + KSLICE_REDUCE_COST_K if pieces else 0)

    base = evaluate({})
    kmax = max(ksum for _, ksum in order)
    cands = []
    for f in (0.75, 0.6, 0.5, 0.4, 0.33, 0.25):  # every tile above a threshold, in equal slices
        if f < KSLICE_FRAC_MIN:
            continue
        thr = max(kmax * f, KSLICE_MIN_K)
        sl = {}
        for gi, ksum in enumerate(ksums):
            s_ = min(KSLICE_MAX_SLICES, -(-ksum // int(thr)), max(1, ksum // KSLICE_MIN_K))
            if s_ > 1:
                sl[gi] = s_
        if sl:
            cands.append(sl)
    per = max(1, slots // T.XCDS)
    single_tile_groups = all(rows <= T.GEMM_BM for _, _, rows in groups)
    for s_ in (2, 3, 4, 6, 8, 12, 16):  # the tiles of each XCD's last, partly filled round
        sl = {}
        for share in T.xcd_shares(order):
            tail_blocks = (len(share) * ct) % per
            if tail_blocks == 0 or tail_blocks * s_ > per + per // 4:
                continue
            for gi, ksum in share[len(share) - (-(-tail_blocks // ct)):]:
                if ksum // s_ >= KSLICE_MIN_K:
                    sl[gi] = s_
        if sl and single_tile_groups:  # (a group = one tile record there: slicing a group slices exactly that tile)
            cands.append(sl)
    best, best_t = None, base
    for sl in cands:
        t = evaluate(sl)
        if t < best_t:
            best, best_t = sl, t
    if best is None or best_t > base * (1.0 - KSLICE_MIN_GAIN):
        return None
    return best


TARGET_BLOCKS = 1536  # blocks a filter-gradient product is split towards
WGRAD_MAX_SPLITS = 64
WGRAD_MIN_SPLITS = 0  # 0 = one split per 64 batch rows once a launch fills the device unsplit


def wgrad_splits(base_blocks, n_pairs, nb):
    """Filter-gradient reduction = S_pix x S_row splits: the pixel-pair list is cut into S_pix contiguous chunks
    and the nb batch rows into S_row ranges (the SAME ranges for every tap).  Tiles are ordered split-major, so each
    XCD streams its own rows of X and dY through its L2 once while all taps consume them (the per-tap
    formulation re-fetched them 10-20x).  Multi-tap levels use row ranges only; single-tap layers also cut the
    pixel list, otherwise the launch would have too few blocks."""
    want = max(1, min(WGRAD_MAX_SPLITS, (TARGET_BLOCKS + base_blocks - 1) // max(base_blocks, 1)))
    max_row = max(1, nb // 64)
    # 64-row ranges also when the unsplit launch already fills the device: with split-major tile order an XCD then streams one
    # row range of X and dY for all taps instead of whole pixel blocks per tap (DUALCNN levels, 165 taps x 10 x 8
    # blocks unsplit: 82 -> 117 TFLOP/s with 8 row ranges)
    if WGRAD_MIN_SPLITS > 0:
        want = max(want, min(WGRAD_MAX_SPLITS, WGRAD_MIN_SPLITS))
    elif base_blocks >= TARGET_BLOCKS:
        want = max(want, min(WGRAD_MAX_SPLITS, max_row))
    s_row = min(want, max_row)
    if s_row >= 5:  # a multiple of 8 row ranges maps whole ranges onto the 8 XCDs
        s_row = min(max(8, max_row // 8 * 8), (s_row + 7) // 8 * 8)
    s_pix = max(1, min(n_pairs, want // s_row))
    return s_pix, s_row
