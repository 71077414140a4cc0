"""Host-side tables of the grouped multi-segment GEMM launches (include/hypel.h: hypel_seg_gemm_f32 and its variants):
the `Launch` record the planner emits, the `GemmShape` of a product, `GemmTables`, the builder of a launch's (groups,
segments, 128-row tile records) arrays incl. the XCD-aware tile order, segment pairing and the algorithmic-byte count of
a launch, and the table halves of the planner's emitters (filter-gradient splits, K-slices, the merged filter-gradient
launch).  Numbers in, tables and entries out: nothing here sees a backend, a session or a `Ref`; which slicing, split or
kernel family a launch gets is decided in gemm_policy."""
from typing import NamedTuple

import numpy as np

from . import abi
from .backend import GEMM_BM, GROUP_DTYPE, MTILE_DTYPE, SEG_DTYPE, TILE_DTYPE, TILE_PLAIN, arg_index

SEG_PAIR_FLAG = abi.const("HYPEL_SEG_PAIR_FLAG")
# flag bits of a launch (include/hypel.h)
GEMM_SINGLE_SEG = abi.const("HYPEL_GEMM_SINGLE_SEG")
GEMM_PAIRED_SEGS = abi.const("HYPEL_GEMM_PAIRED_SEGS")  # (bit of `accumulate`)
GEMM_SPLIT6 = abi.const("HYPEL_GEMM_SPLIT6")  # (bit of `accumulate`)
GEMM_MULTI_SPLIT6 = abi.const("HYPEL_GEMM_MULTI_SPLIT6")  # (bit of hypel_seg_gemm_multi_f32's tile_width)
GEMM_MFMA16X4 = abi.const("HYPEL_GEMM_MFMA16X4")  # 128x64 blocks on the 16x16x4 MFMA (merged level, <= 16 filters)
GEMM_VAR_N = abi.const("HYPEL_GEMM_VAR_N")  # tile records carry their group's column count
XCDS = 8 # the kernels' XCD remap: block b runs on XCD b % 8 and takes record (b % 8) * L + b / 8 of 8 * L records


class GemmShape(NamedTuple):
    """The operands of one grouped product C (+)= op(A) op(B): output columns, leading dimensions, transposes."""
    n: int
    lda: int
    ta: int
    ldb: int
    tb: int
    ldc: int
    a_ks = property(lambda s: s.lda if s.ta else 1)  # element distance of one reduction column in A ...
    b_ks = property(lambda s: 1 if s.tb else s.ldb)  # ... and in B


def xcd_shares(items):
    """Cut a list into eight contiguous shares, the first len % 8 of them one longer: what the XCD remap hands each XCD."""
    q, r = divmod(len(items), XCDS)
    cuts = [x * q + min(x, r) for x in range(XCDS + 1)]
    return [items[cuts[x]:cuts[x + 1]] for x in range(XCDS)]


def xcd_deal(items, weight, loads=None):
    """Deal items heaviest first, each onto the XCD with the least load so far (ties: the lowest index).  loads = what the
    XCDs hold before.  Returns (the eight lists of dealt items, the loads afterwards)."""
    loads = [0] * XCDS if loads is None else list(loads)
    dealt = [[] for _ in range(XCDS)]
    for it in sorted(items, key=lambda it: -weight(it)):
        x = min(range(XCDS), key=lambda i: (loads[i], i))
        dealt[x].append(it)
        loads[x] += weight(it)
    return dealt, loads


class Launch:
    __slots__ = ("name", "args", "flops", "bytes", "tag", "kparts", "meta")

    def __init__(self, name, args, flops=0, nbytes=0, tag=""):
        self.name = name
        self.args = args
        self.flops = flops
        self.bytes = nbytes
        self.tag = tag
        self.kparts = 1  # channel parts the reduction dimension of a level forward was cut into (diagnostic)
        self.meta = {}  # diagnostics (e.g. the products a merged filter-gradient launch contains)

    def set(self, param, value):
        """Replace the argument that include/hypel.h calls `param` in this launch's prototype."""
        i = arg_index(self.name, param)
        self.args = tuple(self.args[:i]) + (value,) + tuple(self.args[i + 1:])


class GemmTables:
    """Host-side builder of the (groups, segments, tiles) tables of one hypel_seg_gemm_f32 launch."""

    def __init__(self):
        self.groups = []  # (c_off, [segs], rows)
        self.keys = []  # optional locality key per group (tiles are ordered key-major)
        self.subkeys = []  # secondary locality key (phase inside a row chunk)
        self.ns = []  # per-group column count (0 = the launch's n): the ring groups of a merged multi-kernel level
        self.flags = []  # per-group hypel_tile_t.flags (TILE_PLAIN: a K-slice partial)
        self.tail = []   # per-group: dealt to the END of the XCDs' work lists (the K-slices of a launch, see finalize)

    def add_group(self, c_off, segs, rows, key=None, subkey=0, n=0, flags=0, tail=False):
        self.groups.append((int(c_off), segs, int(rows)))
        self.keys.append(key)
        self.subkeys.append(subkey)
        self.ns.append(int(n))
        self.flags.append(int(flags))
        self.tail.append(bool(tail))

    def n_of(self, gi, n):
        return self.ns[gi] or n

    def ksum(self, gi):
        return sum(k for _, _, k in self.groups[gi][1])

    def tiles(self):
        """The 128-row tile records (work, group, m0, (locality key: the group's, else the tile's row chunk; sub-key)) in
        group order."""
        return [(self.ksum(gi) * min(GEMM_BM, rows - m0), gi, m0,
                 (self.keys[gi] if self.keys[gi] is not None else m0 // GEMM_BM, self.subkeys[gi]))
                for gi, (_, _, rows) in enumerate(self.groups) for m0 in range(0, rows, GEMM_BM)]

    def tile_order(self):
        """The tile records in dispatch order: row-chunk major, heavy tiles first inside a chunk.  With the kernel's XCD
        remap each XCD works through a contiguous range of this list, i.e. through whole row chunks: the ~49 pixel
        blocks of activations that all the (pixel, branch) tiles of one chunk keep re-reading stay resident in that
        XCD's 4 MB L2.  Filter-gradient launches pass key = split index (= batch-row range), for the same reason."""
        return sorted(self.tiles(), key=lambda t: (t[3], -t[0]))

    def finalize(self, n, pair=False):
        """pair: consecutive segments of a group with k <= 16 each are marked to share one k-tile (SEG_PAIR_FLAG on
        the first; the kernel's data-gradient variant for short segments).  self.paired = number of pairs made."""
        self.paired = 0
        segs = []
        garr = np.zeros(len(self.groups), GROUP_DTYPE)
        macs = 0
        for gi, (c_off, gs, rows) in enumerate(self.groups):
            garr[gi] = (c_off, len(segs), len(gs), rows, 0)
            first = len(segs)
            segs += [(int(a_off), int(b_off), int(k), 0) for (a_off, b_off, k) in gs]
            if pair:
                i = first
                while i + 1 < len(segs):
                    (a0, b0, k0, _), (a1, b1, k1, _) = segs[i], segs[i + 1]
                    if k0 <= 16 and k1 <= 16 and abs(a0 - a1) * 4 < (1 << 31) and abs(b0 - b1) * 4 < (1 << 31):
                        segs[i] = (a0, b0, k0 | SEG_PAIR_FLAG, 0)
                        self.paired += 1
                        i += 2
                    else:
                        i += 1
            macs += rows * self.ksum(gi) * self.n_of(gi, n)
        tiles = self.tile_order()

        def record(g, m0):
            c_off, gs, rows = self.groups[g]
            sb, sc = int(garr[g]["seg_begin"]), len(gs)
            a0, b0, k0 = segs[sb][:3] if sc else (0, 0, 0)  # incl. the pair flag
            return (g, m0, rows, sb, sc, k0, c_off, a0, b0, self.flags[g], self.ns[g])

        if any(self.tail):
            # K-slices (gemm_policy.kslice): the kernel's XCD remap hands XCD x the x-th EIGHTH of the record array, in order.
            # The ordinary tiles keep their order and are cut into eight contiguous shares; the slices -- the small pieces
            # that are to fill the end of the launch -- are dealt heaviest first, by rows x k, onto the XCD with the least
            # work and go to the END of its share; shares are padded with empty records (rows = 0: the block exits) to one
            # length.
            shares = xcd_shares([t for t in tiles if not self.tail[t[1]]])
            dealt, _ = xcd_deal([t for t in tiles if self.tail[t[1]]], lambda t: t[0],
                                [sum(t[0] for t in sh) for sh in shares])
            shares = [sh + d for sh, d in zip(shares, dealt)]
            L = max(len(sh) for sh in shares)
            empty = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
            recs = []
            for sh in shares:
                recs += [record(g, m0) for (_, g, m0, _) in sh] + [empty] * (L - len(sh))
        else:
            recs = [record(g, m0) for (_, g, m0, _) in tiles]
        # + one zero sentinel record: the kernel's look-ahead clamp (seg_gemm.hip) reads segs[seg_begin] also for a group
        # without segments, which for the last group is one record past the real ones
        sarr = np.array(segs + [(0, 0, 0, 0)], SEG_DTYPE)
        tarr = np.array(recs, TILE_DTYPE) if recs else np.zeros(0, TILE_DTYPE)
        return garr, sarr, tarr, macs

    def compulsory_bytes(self, shape):
        """Algorithmic HBM bytes of the launch: every DISTINCT operand element read once, every output element
        written once (overlapping tap windows of A and weights shared by groups count once)."""
        n_launch, lda, ta, ldb, tb, _ = shape

        def union(spans):
            tot, end = 0, None
            for lo, hi in sorted(spans):
                if end is None or lo > end:
                    tot += hi - lo
                    end = hi
                elif hi > end:
                    tot += hi - end
                    end = hi
            return tot

        a_sp, b_sp, c_el = {}, {}, set()
        for gi, (c_off, gs, rows) in enumerate(self.groups):
            n = self.n_of(gi, n_launch)
            c_el.add((c_off, rows, n))
            for a_off, b_off, k in gs:
                if ta:  # A stored [k, rows]
                    a_sp.setdefault((a_off % lda, rows), []).append((a_off // lda, a_off // lda + k))
                else:  # A stored [rows, k]
                    a_sp.setdefault((a_off % lda, k), []).append((a_off // lda, a_off // lda + rows))
                if tb:  # B stored [n, k]
                    b_sp.setdefault((b_off % ldb, k), []).append((b_off // ldb, b_off // ldb + n))
                else:  # B stored [k, n]
                    b_sp.setdefault((b_off % ldb, n), []).append((b_off // ldb, b_off // ldb + k))
        elems = sum(w * union(sp) for (_, w), sp in a_sp.items()) + sum(w * union(sp) for (_, w), sp in b_sp.items())
        elems += sum(rows * gn for _, rows, gn in c_el)
        return 4 * elems


# ---------------------------------------------------------------------------- table halves of the planner's emitters
def group_per_tile(tables, lda, ldc):
    """The same launch with one group per 128-row tile record (A not transposed: rows of A = rows of C)."""
    out = GemmTables()
    for work, gi, m0, key in tables.tiles():
        c_off, gs, rows = tables.groups[gi]
        out.add_group(c_off + m0 * int(ldc), [(a + m0 * int(lda), b, k) for (a, b, k) in gs], min(GEMM_BM, rows - m0),
                      key=key[0], subkey=key[1])
    return out


def wgrad_split_tables(groups, nb, lda, ldb, slab, s_pix, s_row):
    """A filter-gradient product (TowerPlan._emit_wgrad's groups) cut into s_row x s_pix splits: split = (row range, pixel-
    pair chunk), row range major (the XCD-locality key), writes its slab at split * slab; a group with fewer pixel pairs
    than the widest one gets proportionally cut chunks."""
    n_pairs = max(len(prs) for _, prs, _, _ in groups)
    rcuts = [min(nb, (nb * s // s_row + 31) // 32 * 32) for s in range(s_row)] + [nb]
    tb = GemmTables()
    for sr in range(s_row):
        r0, r1 = rcuts[sr], rcuts[sr + 1]
        for sp in range(s_pix):
            p0, p1 = n_pairs * sp // s_pix, n_pairs * (sp + 1) // s_pix
            si = sr * s_pix + sp
            for c_off, prs, rows, gn in groups:
                q0, q1 = len(prs) * p0 // n_pairs, len(prs) * p1 // n_pairs
                segs = [(a + r0 * lda, b + r0 * ldb, r1 - r0) for a, b in prs[q0:q1]] if r1 > r0 else []
                tb.add_group(si * slab + c_off, segs, rows, key=si, n=gn)
    return tb


def kslice_tables(tables, parts, ldc, c_rel, scratch_rel):
    """The tables with the groups of `parts` = {group: its segments cut into slices (gemm_policy.cut_segments)} sliced, +
    the entries of the reduce that adds the partials to the output: slice 0 keeps the group's output, slices >= 1 write
    plain partials to consecutive regions of the scratch buffer.  c_rel / scratch_rel = element distance of the output /
    the scratch buffer from the base the reduce addresses from (the launch addresses from the output)."""
    out = GemmTables()
    entries, spos = [], 0
    for gi, (c_off, gs, rows) in enumerate(tables.groups):
        if gi not in parts:
            out.add_group(c_off, gs, rows, key=tables.keys[gi], subkey=tables.subkeys[gi])
            continue
        region = rows * int(ldc)
        out.add_group(c_off, parts[gi][0], rows, key=tables.keys[gi], subkey=tables.subkeys[gi], tail=True)
        for i, part in enumerate(parts[gi][1:]):
            out.add_group(scratch_rel - c_rel + spos + i * region, part, rows, flags=TILE_PLAIN, tail=True)
        entries.append((scratch_rel + spos, c_rel + c_off, region, region, len(parts[gi]) - 1, 1))
        spos += (len(parts[gi]) - 1) * region
    return out, entries


def merged_wgrad_tables(products, grads0, scratch_rel):
    """One flush of filter gradients: a launch per tile width over the blocks of every product.  products = [dict(tb, n,
    lda, ldb, tag, S, slab, acc, a0, b0, out_base, unpack, col_tiles)]: a0 / b0 / out_base = element distances of the
    operands and the reduction target from the launch's base (grads0: of the gradient buffer; scratch_rel: of the scratch
    the slabs of the S > 1 products fill in order), col_tiles[group] = gemm_policy.col_tiles of the family the caller
    chose, unpack = a merged level's block copies (src, dst, rows, cols, src ld, dst ld, accumulate) or None.
    Block order: the blocks of one (product, split) pair -- all taps and column tiles that read the same batch-row
    range of X and dY -- form a locality group; groups are dealt to the 8 XCDs heaviest first, by their summed work, onto
    the least loaded XCD (each XCD's L2 then streams a row range once for all its taps, and the XCDs finish together),
    and the record array is laid out so that the kernel's XCD remap hands XCD x exactly its list; short lists are padded
    with empty records.  Returns ([dict(width, segs, records, macs, nbytes, tags, blocks, xcd_work)] widest first, reduce
    entries, unpack entries)."""
    spos = 0
    entries, unpacks = [], []
    per_width = {}  # width -> dict(segs, lists, macs, nbytes, tags)
    for e in products:
        n, tb, out_base, up = e["n"], e["tb"], e["out_base"], e["unpack"]
        if up is not None:
            unpacks += [(out_base + so, grads0 + do, rows, cols, sld, dld, acc, 0)
                        for (so, do, rows, cols, sld, dld, acc) in up]
        if e["S"] > 1:
            c_base = scratch_rel + spos
            entries.append((c_base, out_base, e["slab"], e["slab"], e["S"], 0 if up is not None else e["acc"]))
            spos += e["S"] * e["slab"]
            flags = 0
        else:
            c_base = out_base
            flags = 0 if up is not None else e["acc"]
        a0, b0 = e["a0"], e["b0"]
        first_width = None
        loc_groups = {}  # (width, locality key) -> [work, [(work, record)]]
        for gi, (c_off, gs, rows) in enumerate(tb.groups):
            gn = tb.n_of(gi, n)
            tiles = e["col_tiles"][gi]
            ksum = tb.ksum(gi)
            key = tb.keys[gi] if tb.keys[gi] is not None else 0
            seg_begin = {}
            for wdt in sorted({wd for _, wd in tiles}, reverse=True):
                pw = per_width.setdefault(wdt, dict(segs=[], lists=[], macs=0, nbytes=0, tags=[]))
                if first_width is None:
                    first_width = wdt
                if e["tag"] not in pw["tags"]:
                    pw["tags"].append(e["tag"])
                # (a split with no reduction rows still owns its slab: the reduce reads it, so it must be zero)
                seg_begin[wdt] = len(pw["segs"])
                pw["segs"] += [(a0 + int(a_off), b0 + int(b_off), int(k), 0) for (a_off, b_off, k) in gs]
            first = (a0 + int(gs[0][0]), b0 + int(gs[0][1]), int(gs[0][2])) if gs else (0, 0, 0)
            for m0 in range(0, rows, GEMM_BM):
                work = ksum * min(GEMM_BM, rows - m0)
                for n0, wdt in tiles:
                    per_width[wdt]["macs"] += min(GEMM_BM, rows - m0) * ksum * min(wdt & 0xff, gn - n0)
                    recs = loc_groups.setdefault((wdt, key), [0, []])
                    recs[1].append((work, (c_base + int(c_off), first[0], first[1], m0, rows, n0, gn,
                                           seg_begin[wdt], len(gs), first[2], flags, e["lda"], e["ldb"], gn, 0)))
                    recs[0] += work
        if first_width is not None:
            per_width[first_width]["nbytes"] += tb.compulsory_bytes(GemmShape(n, e["lda"], 1, e["ldb"], 0, n))
        for (wdt, _), (wk, r) in loc_groups.items():  # inside a locality group: heavy blocks first
            r.sort(key=lambda t: -t[0])
            per_width[wdt]["lists"].append((wk, [rec for _, rec in r]))
    launches = []
    for width in sorted(per_width, reverse=True):
        pw = per_width[width]
        dealt, xcd_work = xcd_deal(pw["lists"], lambda t: t[0])
        xcd_recs = [[rec for _, r in d for rec in r] for d in dealt]
        L = max(len(r) for r in xcd_recs)
        arr = np.zeros(XCDS * L, MTILE_DTYPE)  # zero record = empty block (rows 0, no segments)
        for x in range(XCDS):
            if xcd_recs[x]:
                arr[x * L:x * L + len(xcd_recs[x])] = np.array(xcd_recs[x], MTILE_DTYPE)
        launches.append(dict(width=width, records=arr, macs=pw["macs"], nbytes=pw["nbytes"], tags=pw["tags"],
                             segs=np.array(pw["segs"] + [(0, 0, 0, 0)], SEG_DTYPE),  # + the zero sentinel record (finalize)
                             blocks=int(sum(len(r) for r in xcd_recs)), xcd_work=[int(w) for w in xcd_work]))
    return launches, entries, unpacks
