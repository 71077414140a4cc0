"""Lower a recorded `Tower` (hypelcnn_amd.graph) to a flat list of HIP kernel launches.

Layout decisions:
  * every patch tensor lives PIXEL-MAJOR in HBM: buffer[p][n][c], p = y*W + x.  A SAME
    convolution is then, per output pixel, a sum over its VALID taps of dense
    [N x Cin] x [Cin x Cout] products on contiguous row blocks: exact-tap work (2 620 instead of
    4 116 (pixel, tap) pairs for the four kernels of a 7x7 level), no im2col buffer, no masks.
  * flatten + fully_connected is the same sum over pixel blocks; the FC weight rows
    [p*C, (p+1)*C) are the "tap" of pixel p, so the reference's (h, w, c) flatten order is kept.
  * channel concat / split / crop are views: producers write at channel offsets, consumers read
    with (pixel map, channel offset).
  * the backward pass is derived here per node (no autograd engine): residual-map gradient,
    two-pass batch-norm/activation backward, data gradient (same GEMM, transposed weights),
    filter gradient (same GEMM, transposed activations, split over batch rows with a
    deterministic second-stage reduction).
"""
import os

import numpy as np

from . import abi, gemm_policy, gemm_tables as T, graph as G
from .backend import COPY_BLOCK_DTYPE, GEMM_BM, REDUCE_ENTRY_DTYPE, Ref
# (the flag bits of the ABI, the tables and the launch record are re-exported: tests and tools reach them through plan;
# how a product is cut into launches -- and every tunable of that -- lives in gemm_policy and is read through it)
from .gemm_tables import (GEMM_MFMA16X4, GEMM_MULTI_SPLIT6, GEMM_PAIRED_SEGS, GEMM_SINGLE_SEG, GEMM_SPLIT6,  # noqa: F401
                          GEMM_VAR_N, SEG_PAIR_FLAG, GemmShape, GemmTables, Launch)

MSE_PARTIALS = abi.const("HYPEL_MSE_PARTIALS")
STAT_CHUNK_ROWS = 256  # upper bound; see stat_chunk_rows()
STAT_BLOCKS = 256            # blocks per 64-column stripe aimed at
WGRAD_ROW_CHUNK = 512
DGRAD_MAX_SEGS = 18  # segments per data-gradient tile (0 = never split)
MAX_TAPS_PER_TILE = 9  # taps per forward tile of a multi-kernel level
L2_CHUNK_BYTES = int(3.5 * (1 << 20))  # X working set an XCD's L2 keeps
TAP_SPLIT_MIN_BATCH = 64  # below this a pixel block has too few rows for splitting to pay
# bias + leaky-ReLU of a normaliser-less fully-connected layer in the product's epilogue (HYPEL_GEMM_ACT_*): no post-op launch
ACT_IN_GEMM = True
SMALL_BN_ROWS = 1024  # hypel_bn_act_small_*: rows kept in registers (32 row lanes x 32 rows)
# Filter gradients have no consumer before the optimiser: instead of one launch (+ one reduce) per layer they are
# collected and go out as ONE hypel_seg_gemm_multi_f32 per tile width (+ ONE hypel_reduce_splits_multi_f32) at the end
# of the backward pass (and at every data-parallel sync point).  A step's twenty ~25 us launch ramps/drains become three.
MERGE_WGRAD = True
DP_SYNC_WORK = 0.5  # share of the filter-gradient work before the sync point
# Gradient buckets of the data-parallel exchange: two by default (one sync point: >= 60 % of the bytes leave under the
# second half of the backward pass).  More buckets are available for large models -- one sync point per DP_BUCKET_BYTES
# once the weight gradients exceed DP_TWO_BUCKET_BYTES -- but every extra sync point flushes the merged filter-gradient
# launch early: measured on the 1-rank RCCL self-test, DUALCNN (1.03 GB of gradients, 357 ms/step) pays +0.7 % for two
# buckets, +3.8 % for five, +4.6 % for eight, while the tail a second bucket leaves exposed is ~410 MB = 2-5 ms (~1 %)
# of ring all-reduce.  Hence off by default (HYPEL_DP_TWO_BUCKET_MB=256 switches the byte rule on).
DP_TWO_BUCKET_BYTES = int(float(os.environ.get("HYPEL_DP_TWO_BUCKET_MB", "1048576")) * (1 << 20))
DP_BUCKET_BYTES = int(float(os.environ.get("HYPEL_DP_BUCKET_MB", "256")) * (1 << 20))
DP_MAX_BUCKETS = 8
# Merged multi-kernel levels (include/hypel.h): the nested branches of a level share one packed weight image
# W_pack[offset][Cin][C]; per output pixel and ring of input offsets ONE product on the column range of the branches
# that contain the ring.  HYPEL_MERGE_LEVELS: comma list of the passes that use it -- "fwd", "dgrad", "wgrad"; default all
# three -- or "0".  A level qualifies with up to MERGE_LEVELS_MAX_COUT filters per branch; per pass:
#   fwd    <= 16 filters on the fp32 kernels (16x16x4 MFMA), <= MERGE_FWD_MAX_COUT_SPLIT on the split-operand kernels;
#          a biased level keeps the unmerged forward
#   dgrad  every qualifying level
#   wgrad  split-operand kernels only, MERGE_WGRAD_MIN_COUT .. MERGE_WGRAD_MAX_COUT filters
# Measured on MI355X (round 4, NOTES 4.A; per-launch and step-level A/B on one box, fp32 kernels): the merged FORWARD pays
# only for levels with <= 16 filters per branch (128x64 blocks on the 16x16x4 MFMA instead of 128x16: 146 -> 128 us); with
# 30 / 60 filters a branch already fills a 32- / 64-column tile, the A stagings per FLOP do not change and the mixed-width
# launch loses 50 - 60 % (380 -> 583 us, 430 -> 687 us).  The merged DATA GRADIENT (49 instead of 84 segments per pixel)
# gains 2 - 7 % per launch.  The merged FILTER GRADIENT moved work between the three tile-width launches without shortening
# their sum (1584 -> 1593 us): removed in round 5, back in round 6 for the split kernels (below).
MERGE_LEVELS = set(x for x in os.environ.get("HYPEL_MERGE_LEVELS", "fwd,dgrad,wgrad").split(",") if x and x != "0")
MERGE_LEVELS_MAX_COUT = 64
# per pass: widest branch (filters) the pass is merged for, taps per merged forward tile, forward tile-width hint
MERGE_PASS_MAX_COUT = {"fwd": 16, "dgrad": 1 << 20, "wgrad": 1 << 20}
# The merged FILTER GRADIENT (round 6, back from f4fd7b4^ for the split kernels): per input offset d ONE product
# dW_pack[d] = sum_p X[p + d]^T dY[p][:, col0:] of C - col0[ring] columns into a dense packed image, scattered into the HWIO
# gradient slots by hypel_copy_blocks_f32.  Columns per product grow from cout to up to 4 cout: the 30-filter level leaves the
# fp32 pipe for every ring but the outermost.  Same box (profiles/r6_exp_merged_wgrad.txt), sum of the four filter-gradient
# launches of the H13 step: unmerged 1 324 us; levels of 60 + 30 filters merged 1 227; all three levels 1 187 (+ ~8 us for the
# scatter); step 5.62 -> 5.53 ms with the first form.  Narrowest / widest branch (filters) it is used for:
MERGE_WGRAD_MIN_COUT = 1
MERGE_WGRAD_MAX_COUT = 64
# ... and for the split-operand kernels, whose cost is dominated by staging A: sharing one staged A tile between the
# branches of a ring pays for wider branches too
# Round 6, same box (profiles/r6_exp_merged_levels_split.txt; one staged + split A tile serves up to four branches):
# the 30-filter level of H13 -- fp32 kernel, unmerged: 411 us + 55 us of partial-copy reduces; merged on the 128x128 split
# blocks with the round-5 chunking (9 taps, two channel parts): 329 + 65; 16 taps per tile and NO channel parts: 328 + 38
# (= -100 us).  It needs the rows-first wave deal of the split kernels (seg_gemm.hip, wave -> (wave % WM, wave / WM): 357 ->
# 329 us; a ring-3 group fills one column tile of four).  The 60-filter level loses merged (371 + 49 vs 362 + 39), the 15-filter level
# loses on the split kernels (128x64 blocks: 145 us vs 135 on the 16x16x4 MFMA): both keep their round-5 forms.
MERGE_FWD_MAX_COUT_SPLIT = 32
MERGE_MAX_TAPS = 0  # 0 = MAX_TAPS_PER_TILE
MERGE_SPLIT_MAX_TAPS = 16  # ... of a merged forward that runs on the split kernels
MERGE_SPLIT_KPARTS = False  # channel parts (L2_CHUNK_BYTES) for a merged forward on the split kernels
MERGE_FWD_HINT = 2


# Same-box A/B of the planner's constants without editing a file: HYPEL_PLAN_SET="GEMM_SPLIT_MIN_N=64,TARGET_BLOCKS=768"
# (integers / floats; names must exist in this module or in gemm_policy, whichever is the constant's one home).  Not read
# by any test or benchmark default.
def _numeric_constants(module_vars):
    return {k for k, v in module_vars.items() if isinstance(v, (bool, int, float)) and not k.startswith("_")}


_both = _numeric_constants(globals()) & _numeric_constants(vars(gemm_policy))
if _both:
    raise ImportError(f"planner constants {sorted(_both)} are defined in hypelcnn_amd.plan AND hypelcnn_amd.gemm_policy: "
                      "a constant has one home")
for _kv in filter(None, os.environ.get("HYPEL_PLAN_SET", "").split(",")):
    _k, _, _v = _kv.partition("=")
    _home = next((m for m in (globals(), vars(gemm_policy)) if _k in _numeric_constants(m)), None)
    if _home is None:
        raise ValueError(f"HYPEL_PLAN_SET: {_k!r} is not a numeric constant of hypelcnn_amd.plan or hypelcnn_amd.gemm_policy")
    _home[_k] = type(_home[_k])(float(_v)) if not isinstance(_home[_k], bool) else bool(int(_v))


def stat_chunk_rows(rows):
    """Rows per partial-reduction block: ~256 blocks per 64-column stripe, between 16 and 256 rows each
    (a thread walks chunk/4 rows serially, so short matrices get short chunks)."""
    c = (rows + STAT_BLOCKS - 1) // STAT_BLOCKS
    c = max(16, min(STAT_CHUNK_ROWS, c))
    return (c + 3) // 4 * 4


class Storage:
    """Where a SymTensor lives for a given batch size."""

    def __init__(self, buf, nb, ld, pixmap, ch_off, c, npix):
        self.buf = buf
        self.nb = nb
        self.ld = ld
        self.pixmap = pixmap
        self.ch_off = ch_off
        self.c = c
        self.npix = npix

    def pix_off(self, p):
        q = p if self.pixmap is None else self.pixmap[p]
        return q * self.nb * self.ld + self.ch_off

    @property
    def contiguous(self):
        return self.pixmap is None

    @property
    def rows(self):
        return self.npix * self.nb


class TowerPlan:
    """Buffers + launch lists of one tower at one batch size."""

    _defer_bias_sums = False  # PhasePlan: bias-gradient chunk sums wait for its one slab-reduction launch

    def __init__(self, tower, nb, session, loss=None, labels_c=None, external_masks=False, seed=1234, global_nb=None,
                 sync_bn=False):
        self.tower = tower
        self.nb = int(nb)
        # data parallel: samples in the GLOBAL batch this rank's nb samples are a shard of (None = nb x world)
        self.global_nb = global_nb
        # synchronised batch norm (optional, training towers of a data-parallel session): batch statistics and the
        # two backward sums run over the global batch -- one small all-gather / all-reduce per BN layer and direction
        dist_ = getattr(session, "dist", None)
        self.sync_bn = bool(sync_bn) and dist_ is not None and tower.is_training
        self.world = dist_[0] if dist_ is not None else 1
        self.sess = session
        self.be = session.backend
        self.training = tower.is_training
        self.loss = loss
        self.external_masks = external_masks
        self.seed = seed
        self.buffers = {}  # name -> flat tensor
        self.tables = []  # keep uploaded tables alive
        self.storage = {}  # id(owner SymTensor) -> Storage (for owners)
        self.grad_written = {}  # id(owner) -> bool
        self.fwd = []
        self.bwd = []
        self.node_aux = {}
        self.mask_bufs = {}
        self.scratch_sizes = {"scratch_partial": 1, "scratch_wgrad": 1, "sums": 2}
        self._pending_scratch = []
        self.param_written = set()  # variables whose gradient was already written in this plan (shared weights)
        self.sync_points = []  # (index into bwd, lo, hi): grads[lo:hi] are final there (data-parallel overlap)
        self._level_layouts = {}  # node index -> packed layout of a merged multi-kernel level, or None
        self._pending_wgrads = []  # filter-gradient products waiting for the next merged launch (_flush_wgrads)
        self._wgrad_flushes = 0  # merged filter-gradient flushes so far (numbers their partials buffers)
        self._kslice_bufs = 0  # K-sliced launches so far (numbers their partials buffers)
        self._build()

    # ---- which variables does this plan train / which tensors need a gradient (overridden by PhasePlan) ----
    def _trains(self, variables):
        return True

    def _needs_grad(self, t):
        return t.owner.needs_grad

    def _param_acc(self, var):
        acc = 1 if var.name in self.param_written else 0
        self.param_written.add(var.name)
        return acc

    # ------------------------------------------------------------------ buffers
    def _alloc(self, name, n, dtype=None):
        import torch
        t = self.be.zeros(max(int(n), 1), dtype or torch.float32)
        self.buffers[name] = t
        return t

    def _ref(self, name, off=0):
        return Ref(self.buffers[name], off)

    def _param_rel(self, ref):
        """Element distance of `ref` from the flat parameter buffer: the base that table-driven launches address from."""
        d = ref.ptr() - Ref(self.sess.params).ptr()
        assert d % 4 == 0
        return d // 4

    def storage_of(self, t):
        own = t.owner
        st = self.storage[id(own)]
        if t.root is None:
            return st
        # (st.ch_off: the owner may itself be a row-block view of a batched application group, PhasePlan)
        return Storage(st.buf, st.nb, st.ld, t.pixmap, st.ch_off + t.ch_off, t.c, t.npix)

    def grad_storage_of(self, t):
        st = self.storage_of(t)
        return Storage("g:" + st.buf, st.nb, st.ld, st.pixmap, st.ch_off, st.c, st.npix)

    def _new_value(self, t, name):
        buf = self._alloc(name, t.npix * self.nb * t.c)
        st = Storage(name, self.nb, t.c, None, 0, t.c, t.npix)
        self.storage[id(t)] = st
        return st

    def _ensure_grad(self, owner):
        st = self.storage[id(owner)]
        gname = "g:" + st.buf
        if gname not in self.buffers:
            self._alloc(gname, owner.npix * self.nb * owner.c)
        self.grad_written.setdefault(id(owner), False)  # (row-block views of a batched group share one gradient buffer)
        return gname

    def _grad_target(self, t):
        """Returns (Storage of the gradient view, accumulate flag) and marks it written; emits a
        zero fill first when the first contribution only covers a view of the buffer."""
        own = t.owner
        self._ensure_grad(own)
        gst = self.grad_storage_of(t)
        written = self.grad_written[id(own)]
        if not written and t.root is not None:
            full = self.storage[id(own)]
            self.bwd.append(Launch("fill_f32", (self._ref(gst.buf, full.ch_off), full.rows * full.ld, 0.0),
                                   tag="zero-grad-view"))
            written = True
        self.grad_written[id(own)] = True
        return gst, 1 if written else 0

    # ------------------------------------------------------------------ parameters
    def _p(self, var):
        return Ref(self.sess.params, var.offset)

    def _g(self, var):
        return Ref(self.sess.grads, var.offset)

    def _s(self, var):
        return Ref(self.sess.state, var.offset)

    @staticmethod
    def _assert_contiguous(vars_):
        for a, b in zip(vars_[:-1], vars_[1:]):
            if b.offset != a.offset + a.size:
                raise RuntimeError(f"variables {a.name} / {b.name} of a merged level are not contiguous")

    # ------------------------------------------------------------------ gemm emission
    # (what a product needs is decided here, per node; how it becomes launches -- split-K, tile width, kernel family,
    # K-slices, filter-gradient splits -- in gemm_policy; the tables are built in gemm_tables.  The emitters below ask the
    # policy, call the table function, allocate, upload, keep the tables alive and append Launches.)
    def nominal_batch(self):
        return gemm_policy.SPLIT_NOMINAL_BATCH

    def _split6(self, tag, tables, shape, flags, paired, in_multi=False):
        return gemm_policy.split6(tag, tables, shape, flags, paired, self.nb, self.nominal_batch(), in_multi=in_multi)

    def _upload(self, array):
        """Upload a host table and keep it alive with the plan."""
        self.tables.append(self.be.upload(array))
        return Ref(self.tables[-1])

    def _emit_gemm(self, lst, tables, shape, a_ref, b_ref, c_ref, bias_ref, accumulate, tag, allow_split=True, res=None,
                   stats=None, pair=False, hint=None, flags=0, kslice=False, sp6=None):
        """res = (ref, ld, start_ref or None): fold a shortcut gradient into the epilogue (hypel_seg_gemm_res_f32).
        stats = floats of the per-tile statistics scratch: hypel_seg_gemm_stats_f32 (single group, no accumulate).
        kslice: the launch may be balanced with K-slice records (dense output, ldc = n).
        sp6: the kernel family, when the caller already chose it (_split6) to shape the tables."""
        n, lda, ta, ldb, tb, ldc = shape
        split = gemm_policy.split_k(tables, shape) if allow_split and res is None else None
        if split is not None:
            stab, S, c_min, count = split
            pos = len(lst)
            self._emit_gemm(lst, stab, shape, a_ref, b_ref, c_ref, None, 0, tag + "/splitk", allow_split=False)
            self._scratch(lst[pos], "c", "scratch_wgrad", S * count)
            l2 = Launch("reduce_splits_f32", (None, count, S, c_ref + c_min, count, int(accumulate), bias_ref, int(n), 0),
                        nbytes=4 * count * (S + 1), tag="splitk-reduce")
            self._scratch(l2, "partial", "scratch_wgrad", S * count)
            lst.append(l2)
            return
        pair = bool(pair and not ta and tb and n > 16 and stats is None)
        if hint is None:
            hint = gemm_policy.tile_hint(tables, shape, res is not None)
        hint = gemm_policy.HINT_OVERRIDE.get(tag, hint)
        single_seg = bool(not ta and all(len(segs) == 1 for _, segs, _ in tables.groups))
        if sp6 is None:
            sp6 = self._split6(tag, tables, shape, flags,
                               pair and any(k <= 16 for _, gs, _ in tables.groups for _, _, k in gs))
        if sp6:
            pair, hint, single_seg = False, sp6, False
        reduce_after = None
        if (sp6 and kslice and stats is None and not flags and int(ldc) == int(n) and not (ta and tb)
                and tables.groups and not any(tables.ns)):
            # (one group per 128-row tile record first: a 1x1 convolution's data gradient is ONE group of 50 176 rows)
            per_tile = tables if ta or all(rows <= GEMM_BM for _, _, rows in tables.groups) else T.group_per_tile(tables, lda, ldc)
            slices = gemm_policy.kslice(per_tile, shape, sp6)
            if slices:
                tables, reduce_after = self._apply_kslices(per_tile, slices, shape, c_ref, tag)
        garr, sarr, tarr, macs = tables.finalize(n, pair=pair)
        if len(tarr) == 0:
            return
        g_r, s_r, t_r = (self._upload(a) for a in (garr, sarr, tarr))
        # the launch's `accumulate` word (include/hypel.h): bit 0, the tile-width hint in bits 8-9, the flag bits
        word = (int(accumulate) | hint << 8 | int(flags) | (GEMM_SPLIT6 if sp6 else 0)
                | (GEMM_PAIRED_SEGS if pair and tables.paired else 0) | (GEMM_SINGLE_SEG if single_seg and not flags else 0))
        args = (a_ref, int(lda), int(ta), b_ref, int(ldb), int(tb), c_ref, int(ldc), int(n), g_r, s_r, t_r,
                int(len(tarr)), bias_ref, word)
        name = "seg_gemm_f32"
        if res is not None:
            name = "seg_gemm_res_f32"
            args = args + (res[0], int(res[1]), res[2])
        elif stats is not None:
            assert len(tables.groups) == 1 and not (word & 1) and int(ldc) == int(n)
            name = "seg_gemm_stats_f32"
            args = args + (None,)
        l = Launch(name, args, flops=2 * macs, nbytes=tables.compulsory_bytes(shape), tag=tag)
        if stats is not None:
            self._scratch(l, "stats_partial", "scratch_partial", stats)
        lst.append(l)
        if reduce_after is not None:
            l.meta["kslices"] = reduce_after.meta["kslices"]
            lst.append(reduce_after)

    def _apply_kslices(self, tables, slices, shape, c_ref, tag):
        """The tables with the chosen groups cut into K-slices + the launch that adds the partials to the output."""
        sname = f"kslice:{self._kslice_bufs}"
        self._kslice_bufs += 1
        self._alloc(sname, sum((s_ - 1) * tables.groups[gi][2] * int(shape.ldc) for gi, s_ in slices.items()))
        parts = {gi: gemm_policy.cut_segments(tables.groups[gi][1], s_, int(shape.a_ks), int(shape.b_ks))
                 for gi, s_ in slices.items()}
        out, entries = T.kslice_tables(tables, parts, shape.ldc, self._param_rel(c_ref), self._param_rel(self._ref(sname)))
        e_r = self._upload(np.array(entries, REDUCE_ENTRY_DTYPE))
        red = Launch("reduce_splits_multi_sized_f32", (Ref(self.sess.params), e_r, len(entries),
                                                       int(max(e[3] for e in entries))),
                     nbytes=4 * sum(cnt * (S + 2) for (_, _, _, cnt, S, _) in entries), tag="kslice-reduce")
        red.meta = {"kslices": {"tiles": len(entries), "slices": int(sum(slices.values())), "of": tag}}
        return out, red

    def _dp_sync_node(self):
        """Data-parallel overlap: [(node index, lo, hi)] -- walking backward, the nodes after which the weight gradients
        at flat offsets [lo, hi) are final.  Small models (H13: 32.6 MB) get ONE point: the node after which >= 60 % of the
        weight-gradient bytes are final; large ones one point per DP_BUCKET_BYTES.  Weights are laid out in creation order
        (Session.finalize_variables), i.e. in node order, so that range is one contiguous tail.
        The merged filter-gradient launch is flushed at this point, so the point also has to cut the filter-gradient
        WORK into two useful halves: at the first node that satisfies the byte rule (H13: fc_0, 75 % of the bytes but 8 %
        of the multiply-adds) the early launch held a handful of badly shaped products and cost 0.13 ms per step; the
        walk therefore continues until >= DP_SYNC_WORK of the filter-gradient multiply-adds are behind it, as long as
        >= 15 % of them -- backward time to hide the all-reduce under -- remain (H13: the first level, 66 % / 34 %)."""
        if os.environ.get("HYPEL_DP_NO_SYNC") == "1":  # diagnostic: one graph, one all-reduce after the backward pass
            return None
        sized = []
        for idx, node in enumerate(self.tower.nodes):
            if isinstance(node, G.LinearNode):
                ws = [b.w for b in node.branches]
                if ws and all(w.trainable and w.offset is not None for w in ws):
                    macs = sum(w.size for w in ws) * max(1, node.out.npix)  # x batch: the same factor for every node
                    sized.append((idx, min(w.offset for w in ws), max(w.offset + w.size for w in ws), macs))
        if len(sized) < 2:
            return None
        total = sum(hi - lo for _, lo, hi, _ in sized)
        total_macs = sum(m for _, _, _, m in sized)
        hi_all = max(hi for _, _, hi, _ in sized)
        if 4 * total > DP_TWO_BUCKET_BYTES:
            # large model: one sync point per DP_BUCKET_BYTES of finished weight gradients (walking backward), the last
            # one early enough that >= 10 % of the filter-gradient work is still ahead to hide it
            n_buckets = max(3, min(DP_MAX_BUCKETS, -(-4 * total // DP_BUCKET_BYTES)))
            points, acc, acc_macs = [], 0, 0
            for k in range(len(sized) - 1, 0, -1):
                idx, lo, hi, macs = sized[k]
                acc += hi - lo
                acc_macs += macs
                tail_lo = min(l for _, l, _, _ in sized[k:])
                contiguous = sum(h - l for _, l, h, _ in sized[k:]) == hi_all - tail_lo
                if not contiguous or acc_macs > 0.9 * total_macs:
                    continue
                if acc >= total * (len(points) + 1) / n_buckets:
                    points.append((idx, tail_lo, hi_all))
                    if len(points) == n_buckets - 1:
                        break
            return points or None
        acc = acc_macs = 0
        best = None
        for k in range(len(sized) - 1, 0, -1):  # never the first layer: nothing would be left to overlap with
            idx, lo, hi, macs = sized[k]
            acc += hi - lo
            acc_macs += macs
            tail_lo = min(l for _, l, _, _ in sized[k:])
            contiguous = sum(h - l for _, l, h, _ in sized[k:]) == hi_all - tail_lo
            if acc >= 0.6 * total and contiguous:
                if best is None:
                    best = (idx, tail_lo, hi_all)
                if acc_macs > 0.85 * total_macs:
                    break  # too little backward left behind this point
                best = (idx, tail_lo, hi_all)
                if acc_macs >= DP_SYNC_WORK * total_macs:
                    break
        return [best] if best is not None else None

    # ------------------------------------------------------------------ consumers / epilogue fusion
    @staticmethod
    def _inputs_of(node):
        if isinstance(node, G.LinearNode):
            return list(node.sources) + [r for r, _ in node.residuals]
        if isinstance(node, G.PostNode):
            return [node.src] + [r for r, _ in node.residuals]
        if hasattr(node, "srcs"):
            return list(node.srcs)
        return [node.src]

    def _build(self):
        tw = self.tower
        nb = self.nb
        # inputs: the loader hands over NHWC batches; keep a persistent staging tensor and convert
        for name, t in tw.inputs.items():
            if t.hw is None:
                self._alloc("in:" + name, nb * t.c)
                self.storage[id(t)] = Storage("in:" + name, nb, t.c, None, 0, t.c, 1)
            else:
                self._alloc("in:" + name, nb * t.npix * t.c)  # NHWC as delivered
                st = self._new_value(t, "pnc:" + name)
                self.fwd.append(Launch("nhwc_to_pnc", (self._ref("in:" + name), self._ref(st.buf), nb, t.npix, t.c,
                                                       st.ld), nbytes=8 * nb * t.npix * t.c, tag="layout"))
        if self.training:
            import torch
            self._alloc("step_ctr", 1, torch.int64)
        pack_pos = len(self.fwd)
        for idx, node in enumerate(tw.nodes):
            if isinstance(node, G.LinearNode):
                self._fwd_linear(idx, node)
            elif isinstance(node, G.PostNode):
                self._fwd_post(idx, node)
            elif isinstance(node, G.LRNNode):
                self._fwd_lrn(idx, node)
            elif isinstance(node, G.CapsuleNode):
                self._fwd_capsule(idx, node)
            elif isinstance(node, G.LabelMaskNode):
                self._fwd_label_mask(idx, node)
            else:
                raise TypeError(node)
        self._emit_level_packs(pack_pos)
        if self.loss is not None:
            self._emit_loss()
        if self.training and self.loss is not None:
            sync_pts = self._dp_sync_node() if getattr(self.sess, "dist", None) is not None else None
            sync_map = {p[0]: p for p in (sync_pts or [])}
            for idx in range(len(tw.nodes) - 1, -1, -1):
                node = tw.nodes[idx]
                if isinstance(node, G.LinearNode):
                    self._bwd_linear(idx, node)
                elif isinstance(node, G.PostNode):
                    self._bwd_post(idx, node)
                elif isinstance(node, G.LRNNode):
                    self._bwd_lrn(idx, node)
                elif isinstance(node, G.CapsuleNode):
                    self._bwd_capsule(idx, node)
                elif isinstance(node, G.LabelMaskNode):
                    self._bwd_label_mask(idx, node)
                if idx in sync_map:
                    # every weight gradient at flat offsets >= lo is final once the side stream is joined: the session
                    # starts the all-reduce of what no earlier point covered here, under the rest of the backward pass
                    sync_at = sync_map[idx]
                    self._flush_wgrads()
                    self.sync_points.append((len(self.bwd), sync_at[1], sync_at[2]))
            self._flush_wgrads()
        # shared scratch (stream order makes reuse safe)
        self._finish_scratch()

    def _finish_scratch(self):
        """Shared scratch (stream order makes reuse safe): allocate every region at its largest request, resolve the
        launches' scratch arguments."""
        for name, size in self.scratch_sizes.items():
            self._alloc(name, size)
        for launch, param, name in self._pending_scratch:
            launch.set(param, self._ref(name))

    def _scratch(self, launch, param, name, size=0):
        """The launch's argument `param` (the header's parameter name) is the shared scratch region `name`."""
        self.scratch_sizes[name] = max(self.scratch_sizes.get(name, 1), int(size))
        self._pending_scratch.append((launch, param, name))

    # ------------------------------------------------------------------ LinearNode forward
    def _vec_params(self, node):
        """Concatenated per-channel vectors of a (possibly merged) node."""
        brs = node.branches
        aux = {}
        if node.has_bn:
            for i, key in enumerate(("beta", "mm", "mv")):
                vs = [b.bn[i] for b in brs]
                self._assert_contiguous(vs)
                aux[key] = vs[0]
        if node.has_bias:
            vs = [b.bias for b in brs]
            self._assert_contiguous(vs)
            aux["bias"] = vs[0]
        ws = [b.w for b in brs]
        self._assert_contiguous(ws)
        aux["w0"] = ws[0]
        aux["wsize"] = sum(w.size for w in ws)
        return aux

    # ------------------------------------------------------------------ merged multi-kernel levels
    def _level_layout(self, idx, node):
        """Packed layout of a multi-kernel level whose branches are nested odd kernels of equal width on one contiguous
        source (HYPELCNNModel.py:167-183), or None.  An input offset (dy, dx) at ring r = max(|dy|, |dx|) belongs to the
        branches with (k - 1) / 2 >= r -- a suffix of the concat order -- i.e. to the output columns [col0[r], C).
        Offsets are numbered ring-major; W_pack[d] is [Cin x C] (columns below col0 are never touched)."""
        if idx in self._level_layouts:
            return self._level_layouts[idx]
        lay = None
        brs = node.branches
        # (a biased level -- DUALCNN -- keeps its unmerged forward: the bias rides in the GEMM epilogue / the tap-split
        # reduce; its data and filter gradients do not see the bias at all)
        if (MERGE_LEVELS and node.kind == "conv" and len(brs) >= 2
                and self.nb >= TAP_SPLIT_MIN_BATCH and len(node.sources) == 1):
            ks = [b.k for b in brs]
            co = brs[0].cout
            src = node.sources[0]
            ok = (all(k % 2 == 1 for k in ks) and all(a < b for a, b in zip(ks, ks[1:])) and
                  all(b.cout == co for b in brs) and co <= MERGE_LEVELS_MAX_COUT and src.hw is not None and
                  self.storage_of(src).contiguous)
            if ok:
                rmax = (ks[-1] - 1) // 2
                first = [next(i for i, k in enumerate(ks) if (k - 1) // 2 >= r) for r in range(rmax + 1)]
                offs = []
                for r in range(rmax + 1):
                    offs += [(dy, dx, r) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if max(abs(dy), abs(dx)) == r]
                C = co * len(brs)
                lay = dict(offs=offs, index={(dy, dx): d for d, (dy, dx, _) in enumerate(offs)}, rmax=rmax, first=first,
                           col0=[f * co for f in first], co=co, C=C, cin=src.c, buf=f"wpack:{idx}", dense_off=[],
                           has_bias=node.has_bias)
                pos = 0
                for (_, _, r) in offs:  # dense image of the packed filter gradient: [d] -> [Cin x (C - col0[r])]
                    lay["dense_off"].append(pos)
                    pos += src.c * (C - lay["col0"][r])
                lay["dense_size"] = pos
                assert pos == sum(b.w.size for b in brs)
        self._level_layouts[idx] = lay
        if lay is not None and (self._level_pass(idx, node, "fwd") or self._level_pass(idx, node, "dgrad")):
            # these passes read the packed image (the filter gradient does not)
            lay["packed"] = True
            self._alloc(lay["buf"], len(lay["offs"]) * lay["cin"] * lay["C"])
        return lay

    def _level_pass(self, idx, node, what):
        """The level's packed layout if pass `what` ("fwd" / "dgrad" / "wgrad") uses the merged form, else None."""
        lay = self._level_layout(idx, node)
        cap = MERGE_PASS_MAX_COUT[what]
        if what == "fwd" and gemm_policy.GEMM_SPLIT == 6:
            cap = max(cap, MERGE_FWD_MAX_COUT_SPLIT)
        if lay is None or what not in MERGE_LEVELS or lay["co"] > cap or (what == "fwd" and lay["has_bias"]):
            return None
        if what == "wgrad" and not (gemm_policy.GEMM_SPLIT == 6 and MERGE_WGRAD and MERGE_WGRAD_MIN_COUT <= lay["co"] <= MERGE_WGRAD_MAX_COUT):
            return None  # (on the fp32 kernels it moved work between the width classes without shortening their sum, NOTES 4.A)
        return lay

    def _emit_level_packs(self, pos):
        """ONE hypel_copy_blocks_f32 in front of the forward pass (inserted at launch position `pos`): every
        (branch, tap) slice [Cin x cout] of every merged level goes to its offset / column range of the level's packed
        image (the variables keep their TF layouts)."""
        base = Ref(self.sess.params)
        ents = []
        for idx, node in enumerate(self.tower.nodes):
            lay = self._level_layouts.get(idx)
            if lay is None or not lay.get("packed"):
                continue
            dst0 = self._param_rel(self._ref(lay["buf"]))
            cin, co, C = lay["cin"], lay["co"], lay["C"]
            ents += [(w_, dst0 + lay["index"][(dy, dx)] * cin * C + col, cin, co, co, C, 0, 0)
                     for dy, dx, w_, col, _ in self._taps(self._columns(node), cin)]
        if not ents:
            return
        self.fwd.insert(pos, Launch("copy_blocks_f32", (base, self._upload(np.array(ents, COPY_BLOCK_DTYPE)), len(ents),
                                                        max(e[2] * e[3] for e in ents)),
                                    nbytes=8 * sum(e[2] * e[3] for e in ents), tag="level-pack"))

    # ------------------------------------------------------------------ convolution taps
    @staticmethod
    def _columns(node):
        """[(branch, its first output column)] in concat order."""
        cols, col = [], 0
        for b in node.branches:
            cols.append((b, col))
            col += b.cout
        return cols

    @staticmethod
    def _taps(branches, cin, lay=None):
        """The taps of a convolution as (dy, dx, w, col, n): input offset, element offset of the tap's [cin x n] weight
        block (at its first column) in the buffer the pass reads, and the output columns [col, col + n) of Y / dY it covers.
        branches = [(branch, col)]: taps in branch order, (i, j) row-major, in the parameter buffer.  A merged level (lay):
        its ring-major input offsets over the packed image W_pack[d] = [cin x C] (wpack:<idx>), columns [col0[ring], C)."""
        if lay is not None:
            C, col0 = lay["C"], lay["col0"]
            return [(dy, dx, d * cin * C + col0[r], col0[r], C - col0[r]) for d, (dy, dx, r) in enumerate(lay["offs"])]
        return [(i - (b.k - 1) // 2, j - (b.k - 1) // 2, b.w.offset + (i * b.k + j) * cin * b.cout, col, b.cout)
                for b, col in branches for i in range(b.k) for j in range(b.k)]

    @staticmethod
    def _fwd_segs(taps, s_st, h, w, p, wo=None, r=0):
        """Forward segments of output pixel p: one per tap that reads a real input pixel, over all Cin reduction columns.
        VALID padding: the output is (h - 2r) x wo pixels and output pixel (y, x) is centred on input pixel (y + r, x + r)."""
        py, px = divmod(p, w if wo is None else wo)
        py, px = py + r, px + r
        return [(s_st.pix_off((py + dy) * w + px + dx), w_, s_st.c) for dy, dx, w_, _, _ in taps
                if 0 <= py + dy < h and 0 <= px + dx < w]

    @staticmethod
    def _valid_geometry(node):
        """(output width, ring) of a convolution: (None, 0) with SAME padding; VALID: output pixel (y, x) of the
        (h - 2r) x (w - 2r) map reads the window centred on input pixel (y + r, x + r)."""
        if not node.valid:
            return None, 0
        return node.out.hw[1], (node.branches[0].k - 1) // 2

    @staticmethod
    def _partial_copies(segs, S, kp_n=1, ldb=0):
        """One output group's segments [(a_off, b_off, k)] cut into kp_n channel parts -- every segment's reduction columns
        cut at multiples of 16, B advancing ldb elements per column -- and each part into S contiguous chunks of segments.
        Yields (kp, si, chunk), channel part major; each writes its own partial copy of the group's output."""
        def cut(k, q):
            return k if q == kp_n else min(k, (k * q // kp_n + 15) // 16 * 16)

        for kp in range(kp_n):
            part = [(a + cut(k, kp), b + cut(k, kp) * ldb, cut(k, kp + 1) - cut(k, kp)) for a, b, k in segs]
            for si in range(S):
                yield kp, si, part[len(part) * si // S:len(part) * (si + 1) // S]

    @staticmethod
    def _channel_parts(cin, h, w):
        """L2 locality: the tiles of one 128-row chunk re-read the chunk's pixel blocks of X once per tap.  When those
        blocks (pixels x 128 rows x Cin) exceed what an XCD's 4 MB L2 keeps, every tap goes back to HBM (measured: 1.56 GB
        fetched for 117 MB of operands at Cin = 240).  The reduction dimension is then cut into this many channel parts,
        processed one after the other inside a chunk (tile order key), each writing its own partial copy like a tap chunk."""
        return max(1, min(4, -(-(h * w * GEMM_BM * cin * 4) // L2_CHUNK_BYTES), cin // 16))

    def _reduce_tap_copies(self, ybuf, rows, c, col, n, copies, bias=None):
        """Add partial copies 1 .. copies - 1 of the output columns [col, col + n) -- stored behind Y in `ybuf`, rows x c
        each -- into copy 0 = Y (+ bias: every partial copy would have added it)."""
        if copies > 1:
            self.fwd.append(Launch("reduce_splits_f32", (self._ref(ybuf, rows * c + col), rows * c, copies - 1,
                                                         self._ref(ybuf, col), rows * n, 1, bias, n, c),
                                   nbytes=4 * rows * n * (copies + 1), tag="tap-split-reduce"))

    def _fwd_level_merged(self, node, lay, s_st, ybuf, c, h, w):
        """Forward pass of a merged level: per output pixel and ring r the product
        Y[p][:, col0[r]:] (+)= sum_{d in ring r, valid} X[p + d] . W_pack[d][:, col0[r]:].  The kernel family is chosen on
        these products (their MACs do not depend on how they are cut); rings with more offsets than that family's taps per
        tile are cut into chunks, and on the fp32 kernels the reduction into channel parts.  Every (ring chunk, channel
        part) writes its own copy of Y (copy 0 is Y itself), summed per branch as for the tap splits of the unmerged form."""
        nb, C = self.nb, lay["C"]
        rows_all = node.out.npix * nb
        taps = self._taps(self._columns(node), lay["cin"], lay)
        rings = [[t for t, o in zip(taps, lay["offs"]) if o[2] == r] for r in range(lay["rmax"] + 1)]
        whole = GemmTables()  # one group per (pixel, ring), pixel major
        for p in range(h * w):
            for ring in rings:
                whole.add_group(p * nb * c + ring[0][3], self._fwd_segs(ring, s_st, h, w, p), nb, n=ring[0][4])
        flags = GEMM_VAR_N | (GEMM_MFMA16X4 if lay["co"] <= 16 and C <= 64 else 0)
        tag = f"fwd:{node.branches[0].scope}/merged"
        shape = GemmShape(n=C, lda=s_st.ld, ta=0, ldb=C, tb=0, ldc=c)
        sp6 = self._split6(tag, whole, shape, flags, False)
        max_taps = MERGE_MAX_TAPS or (MERGE_SPLIT_MAX_TAPS if sp6 else MAX_TAPS_PER_TILE)
        S_r = [max(1, -(-len(ring) // max_taps)) for ring in rings]
        kp_n = self._channel_parts(lay["cin"], h, w) if not sp6 or MERGE_SPLIT_KPARTS else 1
        chunk0 = [sum(S_r[:r]) for r in range(len(rings) + 1)]  # first chunk index of ring r
        if chunk0[-1] * kp_n > 1:
            self._alloc(ybuf, rows_all * c * chunk0[-1] * kp_n)
        tb = GemmTables()
        for gi, (c_off, segs, _) in enumerate(whole.groups):
            r = gi % len(rings)
            for kp, si, chunk in self._partial_copies(segs, S_r[r], kp_n, C):
                tb.add_group(((chunk0[r] + si) * kp_n + kp) * rows_all * c + c_off, chunk, nb, subkey=kp, n=whole.ns[gi])
        pos = len(self.fwd)
        self._emit_gemm(self.fwd, tb, shape, self._ref(s_st.buf), self._ref(lay["buf"]), self._ref(ybuf), None, 0, tag,
                        allow_split=False, hint=MERGE_FWD_HINT, flags=flags,
                        sp6=sp6)  # (a split-operand launch takes its own width, gemm_policy.split6_width)
        if len(self.fwd) > pos:
            self.fwd[pos].kparts = kp_n
        for b, col in self._columns(node):  # the copies that hold columns of branch b: 0 .. chunk0[ring of b + 1] * kp_n - 1
            self._reduce_tap_copies(ybuf, rows_all, c, col, b.cout, chunk0[(b.k - 1) // 2 + 1] * kp_n)

    def _fwd_conv(self, node, aux, s_st, ybuf, c, h, w, bias_ref):
        """Forward pass of a convolution, per branch.  Tap splitting: a block that walks all 49 taps of a 7x7 branch runs
        ~4x longer than the average tile and finishes alone at ~40 % MFMA utilisation.  Branches with more than
        MAX_TAPS_PER_TILE taps have their tap list cut into S chunks (x the level's channel parts); chunk s writes a partial
        copy Y_s of the output (same layout, stored behind Y in the same buffer) and a strided reduce adds Y_1.. into Y."""
        nb, cin = self.nb, s_st.c
        rows_all = node.out.npix * nb
        splits = {}
        kparts = 1
        if nb >= TAP_SPLIT_MIN_BATCH:
            for b in node.branches:
                taps = min(b.k, h) * min(b.k, w)
                if taps > MAX_TAPS_PER_TILE:
                    splits[id(b)] = (taps + MAX_TAPS_PER_TILE - 1) // MAX_TAPS_PER_TILE
            if splits:
                kparts = self._channel_parts(cin, h, w)
                if kparts > 1:
                    for b in node.branches:
                        if b.k > 1:
                            splits[id(b)] = splits.get(id(b), 1) * kparts
        s_max = max(splits.values()) if splits else 1
        if s_max > 1:
            self._alloc(ybuf, rows_all * c * s_max)
        by_cout = {}
        for b, col in self._columns(node):
            # with a bias, split branches go into a launch of their own (no bias in the GEMM: the reduce adds it)
            by_cout.setdefault((b.cout, bias_ref is not None and splits.get(id(b), 1) > 1), []).append((b, col))
        # batch-norm statistics in the epilogue: a lone 1x1 branch on contiguous input writes ONE [rows x c] matrix
        fuse_stats = (node.has_bn and node.training and len(node.branches) == 1
                      and node.branches[0].k == 1 and s_st.contiguous and s_max == 1 and c > 16
                      and not self._small_bn(node, rows_all))
        aux["stats_in_gemm"] = fuse_stats
        for (cout, split_launch), items in by_cout.items():
            tb = GemmTables()
            kp_used = 1
            for b, col in items:
                if b.k == 1 and s_st.contiguous:
                    tb.add_group(col, [(s_st.pix_off(0), b.w.offset, cin)], rows_all)
                    continue
                S = splits.get(id(b), 1)
                kp_n = kparts if S >= kparts and S % kparts == 0 and kparts > 1 else 1
                kp_used = max(kp_used, kp_n)
                S_tap = S // kp_n
                taps = self._taps([(b, col)], cin)
                wo, vr = self._valid_geometry(node)
                for p in range(node.out.npix):
                    for kp, si, chunk in self._partial_copies(self._fwd_segs(taps, s_st, h, w, p, wo, vr), S_tap, kp_n,
                                                              cout):
                        tb.add_group((kp * S_tap + si) * rows_all * c + p * nb * c + col, chunk, nb, subkey=kp)
            # the kernel indexes bias by (c_off % ldc) + column, so merged branches share one launch
            pos = len(self.fwd)
            self._emit_gemm(self.fwd, tb, GemmShape(n=cout, lda=s_st.ld, ta=0, ldb=cout, tb=0, ldc=c), self._ref(s_st.buf),
                            Ref(self.sess.params), self._ref(ybuf), None if split_launch else bias_ref, 0,
                            f"fwd:{items[0][0].scope}" + ("/split" if split_launch else ""), allow_split=False,
                            stats=((rows_all + GEMM_BM - 1) // GEMM_BM) * 2 * c if fuse_stats else None)
            if len(self.fwd) > pos:
                self.fwd[pos].kparts = kp_used
            for b, col in items:
                self._reduce_tap_copies(ybuf, rows_all, c, col, cout, splits.get(id(b), 1),
                                        None if bias_ref is None else bias_ref + col)

    def _fwd_linear(self, idx, node):
        nb = self.nb
        out = node.out
        c = node.cout
        aux = self._vec_params(node)
        self.node_aux[idx] = aux
        ybuf = f"y:{idx}"
        self._alloc(ybuf, out.npix * nb * c)
        y_st = Storage(ybuf, nb, c, None, 0, c, out.npix)
        aux["y"] = y_st
        bias_ref = self._p(aux["bias"]) if node.has_bias else None

        if node.kind == "conv":
            s_st = self.storage_of(node.sources[0])
            h, w = node.sources[0].hw
            lay = self._level_pass(idx, node, "fwd")
            if lay is not None:
                aux["stats_in_gemm"] = False
                self._fwd_level_merged(node, lay, s_st, ybuf, c, h, w)
            else:
                self._fwd_conv(node, aux, s_st, ybuf, c, h, w, bias_ref)
        elif node.kind == "blockdense":
            # P independent small dense maps (one per band slice) as ONE grouped GEMM: group p reads the source columns
            # of its slice, multiplies by its own weights and writes columns [p*cout, (p+1)*cout) of the output
            src = node.sources[0]
            s_st = self.storage_of(src)
            cout = node.branches[0].cout
            tb = GemmTables()
            for pi, (off, width) in enumerate(node.in_slices):
                tb.add_group(pi * cout, [(s_st.pix_off(0) + off, node.branches[pi].w.offset, width)], nb)
            act_flag = self._act_in_gemm(node, cout)
            aux["act_in_gemm"] = bool(act_flag)
            self._emit_gemm(self.fwd, tb, GemmShape(n=cout, lda=s_st.ld, ta=0, ldb=cout, tb=0, ldc=c), self._ref(s_st.buf),
                            Ref(self.sess.params), self._ref(ybuf), bias_ref, 0,
                            f"fwd:{node.branches[0].scope}+{len(node.branches) - 1}", allow_split=False, flags=act_flag)
        else:  # dense
            b = node.branches[0]
            rowbase = 0
            for si, src in enumerate(node.sources):
                s_st = self.storage_of(src)
                tb = GemmTables()
                segs = [(s_st.pix_off(p), b.w.offset + (rowbase + p * src.c) * c, src.c) for p in range(src.npix)]
                tb.add_group(0, segs, nb)
                shape = GemmShape(n=c, lda=s_st.ld, ta=0, ldb=c, tb=0, ldc=c)
                act_flag = 0
                if len(node.sources) == 1 and gemm_policy.split_k(tb, shape) is None:
                    act_flag = self._act_in_gemm(node, c)
                aux["act_in_gemm"] = bool(act_flag)
                self._emit_gemm(self.fwd, tb, shape, self._ref(s_st.buf), Ref(self.sess.params), self._ref(ybuf),
                                bias_ref if si == 0 else None, 1 if si > 0 else 0, f"fwd:{b.scope}", flags=act_flag)
                rowbase += src.npix * src.c

        rows = out.npix * nb
        # ---- batch-norm statistics ----
        if node.has_bn:
            self._alloc(f"mean:{idx}", c)
            self._alloc(f"rstd:{idx}", c)
            if node.training and self._small_bn(node, rows):
                # short matrix (rows = batch): statistics + finaliser + activation in ONE launch (_emit_post_fwd)
                aux["small_bn"] = True
                aux["mean"] = self._ref(f"mean:{idx}")
            elif node.training and aux.get("stats_in_gemm"):
                # the GEMM left one (mean, M2) pair per 128-row tile: only the finaliser remains
                n_chunks = (rows + GEMM_BM - 1) // GEMM_BM
                self._emit_bn_finalize(idx, node, aux, n_chunks, GEMM_BM, rows, c)
                aux["mean"] = self._ref(f"mean:{idx}")
            elif node.training:
                chunk = stat_chunk_rows(rows)
                n_chunks = (rows + chunk - 1) // chunk
                l1 = Launch("col_stats_partial", (self._ref(ybuf), c, rows, c, chunk, None),
                            nbytes=4 * rows * c, tag="bn-stats")
                self._scratch(l1, "partial", "scratch_partial", n_chunks * 2 * c)
                self.fwd.append(l1)
                self._emit_bn_finalize(idx, node, aux, n_chunks, chunk, rows, c)
                aux["mean"] = self._ref(f"mean:{idx}")
            else:
                self.fwd.append(Launch("rstd_from_var", (self._s(aux["mv"]), c, float(node.bn_eps),
                                                         self._ref(f"rstd:{idx}")), tag="bn-infer"))
                aux["mean"] = self._s(aux["mm"])
            aux["rstd"] = self._ref(f"rstd:{idx}")
            aux["beta_ref"] = self._p(aux["beta"])
        # ---- fused post-op ----
        if node.has_post and aux.get("act_in_gemm"):
            # the product's epilogue already applied bias + leaky-ReLU: the "pre-activation" buffer holds the layer output
            # (the backward kernels take act' from its sign, which a positive slope preserves)
            self.storage[id(out)] = y_st
        elif node.has_post:
            zbuf = f"z:{idx}"
            self._alloc(zbuf, rows * c)
            self.storage[id(out)] = Storage(zbuf, nb, c, None, 0, c, out.npix)
            self._emit_post_fwd(idx, node, self._ref(ybuf), c, rows, c, aux, self._ref(zbuf))
        else:
            self.storage[id(out)] = y_st

    def _act_in_gemm(self, node, n):
        """HYPEL_GEMM_ACT_* code when this layer's post-op is nothing but (bias +) leaky-ReLU of a slope the library names
        (include/hypel.h) and its product runs on the 32-wide matrix-core tiles: a tf_slim.fully_connected without a
        normaliser then is ONE launch.  0: keep the separate post-op launch."""
        act = node.act
        if not (ACT_IN_GEMM and node.has_post and not node.has_bn and not node.residuals and node.dropout_keep is None
                and act is not None and act.code == 1 and n > 16 and not self.sync_bn):
            return 0
        for code, slope in ((1, 0.1), (2, 0.18), (3, 0.2), (4, 0.01)):
            if np.float32(act.alpha) == np.float32(slope):
                return code << 16
        return 0

    def _emit_bn_finalize(self, idx, node, aux, n_chunks, chunk, rows, c):
        """Chunk partials (in scratch_partial) -> mean / rstd / moving averages.  Synchronised batch norm: the rank's
        partials are merged into one (mean, M2, rows) record, the records of all ranks are all-gathered (a host-side
        collective between two graph segments) and merged in rank order."""
        mean_ref, rstd_ref = self._ref(f"mean:{idx}"), self._ref(f"rstd:{idx}")
        tail = (float(node.bn_eps), mean_ref, rstd_ref, self._s(aux["mm"]), self._s(aux["mv"]), self._bn_decay(node))
        if not self.sync_bn:
            l2 = Launch("bn_finalize", (None, n_chunks, chunk, rows, c) + tail, tag="bn-finalize")
            self._scratch(l2, "partial", "scratch_partial", n_chunks * 2 * c)
            self.fwd.append(l2)
            return
        rec = 2 * c + 1
        l2 = Launch("bn_merge_partials", (None, n_chunks, chunk, rows, c, None), tag="bn-sync-merge")
        self._scratch(l2, "partial", "scratch_partial", n_chunks * 2 * c)
        self._scratch(l2, "out", "sbn_local", rec)
        l3 = Launch("_allgather", (None, rec, None), tag="bn-sync-gather")
        self._scratch(l3, "src", "sbn_local", rec)
        self._scratch(l3, "dst", "sbn_all", self.world * rec)
        l4 = Launch("bn_finalize_ranks", (None, self.world, c) + tail, tag="bn-finalize")
        self._scratch(l4, "gathered", "sbn_all", self.world * rec)
        self.fwd += [l2, l3, l4]

    @staticmethod
    def _bn_decay(node):
        """Decay of the moving averages; a node that normalises with batch statistics but must leave the moving averages
        alone (graph.conv2d, normalizer_params["update_moving"] = False) passes 1: m * 1 + batch * 0 = m, bit for bit."""
        return float(node.bn_decay) if node.bn_update else 1.0

    def _mask_ref(self, idx, node, rows, c):
        if node.dropout_keep is None:
            return None
        name = f"mask:{idx}"
        self._alloc(name, rows * c)
        self.mask_bufs[node.dropout_index] = name
        if not self.external_masks:
            self.fwd.append(Launch("dropout_mask", (self._ref(name), rows * c, float(node.dropout_keep),
                                                    int(self.seed * 1000003 + idx), self._ref("step_ctr")), tag="rng"))
        else:
            self.buffers[name].fill_(1.0)
        return self._ref(name)

    def _res_args(self, node):
        out = []
        for (src, ridx) in node.residuals:
            st = self.storage_of(src)
            if not st.contiguous:
                raise NotImplementedError("residual source must cover the same pixels")
            iref = None
            if ridx is not None:
                iref = self._upload(np.asarray(ridx, np.int32))
            out.append((self._ref(st.buf, st.ch_off), st.ld, iref))
        while len(out) < 2:
            out.append((None, 0, None))
        return out

    def _small_bn(self, node, rows):
        """Batch norm over a short matrix (the fully-connected tail: rows = batch) with no shortcut to add: one block
        per channel stripe covers every row, so the whole BN + activation is one launch per direction."""
        return (rows <= SMALL_BN_ROWS and not node.residuals and node.has_post
                and not (self.sync_bn and node.has_bn))

    def _emit_post_fwd(self, idx, node, y_ref, ldy, rows, c, aux, z_ref):
        has_bn = isinstance(node, G.LinearNode) and node.has_bn
        mask = self._mask_ref(idx, node, rows, c)
        aux["mask"] = mask
        (r1, ld1, i1), (r2, ld2, i2) = self._res_args(node)
        act = node.act
        if aux.get("small_bn"):
            self.fwd.append(Launch("bn_act_small_fwd", (
                y_ref, ldy, rows, c, float(node.bn_eps), aux["beta_ref"], act.code if act else 0,
                act.alpha if act else 0.0, mask, c, aux["mean"], aux["rstd"], self._s(aux["mm"]), self._s(aux["mv"]),
                self._bn_decay(node), z_ref, c), nbytes=12 * rows * c, tag="post-fwd-small"))
            return
        self.fwd.append(Launch("bn_act_fwd", (
            y_ref, ldy, rows, c, aux.get("mean") if has_bn else None, aux.get("rstd") if has_bn else None,
            aux.get("beta_ref") if has_bn else None, act.code if act else 0, act.alpha if act else 0.0, mask, c,
            r1, ld1, i1, r2, ld2, i2, z_ref, c), nbytes=4 * rows * c * (2 + len(node.residuals)), tag="post-fwd"))

    def _fwd_post(self, idx, node):
        src, out = node.src, node.out
        s_st = self.storage_of(src)
        if not s_st.contiguous:
            raise NotImplementedError
        rows, c = out.npix * self.nb, out.c
        st = self._new_value(out, f"z:{idx}")
        aux = {}
        self.node_aux[idx] = aux
        self._emit_post_fwd(idx, node, self._ref(s_st.buf, s_st.ch_off), s_st.ld, rows, c, aux, self._ref(st.buf))

    def _fwd_lrn(self, idx, node):
        src, out = node.src, node.out
        s_st = self.storage_of(src)
        rows, c = out.npix * self.nb, out.c
        st = self._new_value(out, f"z:{idx}")
        self.fwd.append(Launch("lrn_fwd", (self._ref(s_st.buf, s_st.ch_off), s_st.ld, rows, c, node.radius,
                                           float(node.bias), float(node.alpha), float(node.beta), self._ref(st.buf), c),
                               nbytes=8 * rows * c, tag="lrn"))

    # ------------------------------------------------------------------ loss
    def _emit_loss(self):
        loss = self.loss
        ps = loss.per_sample
        nb = self.nb
        logits = ps.logits
        l_st = self.storage_of(logits)
        lab = ps.labels
        lab_st = self.storage_of(lab)
        self._alloc("loss_ps", nb)
        self._alloc("loss_ce", 1)
        self._alloc("loss_mse", 1)
        dl = None
        lddl = 0
        if self.training:
            gst, acc = self._grad_target(logits)
            assert acc == 0
            dl, lddl = self._ref(gst.buf, gst.ch_off), gst.ld
        # data parallel: the gradient of the GLOBAL mean loss = sum over ranks of (nb_rank / nb_global) x the local
        # mean-loss gradients (= 1/world for equal shards; the ragged last batch of an epoch-limited run gives ranks
        # unequal shards).  The factor goes in here, at the source, so the exchange is a plain SUM all-reduce with no
        # rescaling pass over the 32 MB buffer afterwards (the reported loss values stay local means)
        dist = getattr(self.sess, "dist", None)
        gworld = 1.0
        if dist is not None:
            gworld = nb / float(self.global_nb) if self.global_nb else 1.0 / dist[0]
        self.fwd.append(Launch("softmax_xent", (self._ref(l_st.buf, l_st.ch_off), l_st.ld, nb, logits.c,
                                                self._ref(lab_st.buf), lab_st.ld, self._ref("loss_ps"), dl, lddl,
                                                gworld / nb), tag="loss"))
        guard = self.sess.guard_ref() if self.training and hasattr(self.sess, "guard_ref") else None
        # the dropout step counter advances once per training step, after the last mask of the step was drawn (masks
        # are drawn in the forward pass): it rides in the loss finaliser
        step = None
        if self.training and self.tower.n_dropout and not self.external_masks:
            step = self._ref("step_ctr")
        mse_args = None
        if ps.extra_mse is not None:
            m = ps.extra_mse
            a_st = self.storage_of(m.a)
            src = m.b.sources[0]  # flatten(image_original): the NHWC staging tensor already has (h, w, c) order
            assert src.node is None and src.root is None, "reconstruction target must be the network input"
            feat = src.npix * src.c
            assert feat == m.a.c
            da, ldda = None, 0
            if self.training:
                gst, acc = self._grad_target(m.a)
                assert acc == 0
                da, ldda = self._ref(gst.buf), gst.ld
            mse_args = (self._ref(a_st.buf), a_st.ld, self._ref("in:" + src.name), feat, nb, feat)
        # xent rows + MSE block partials -> ONE finaliser (means, non-finite flag, step counter)
        ws = None
        if mse_args is not None:
            self._alloc("mse_ws", MSE_PARTIALS)
            ws = self._ref("mse_ws")
            self.fwd.append(Launch("mse_partial_f32", mse_args + (da, ldda, gworld, ws), nbytes=12 * nb * feat,
                                   tag="loss"))
        self.fwd.append(Launch("loss_finalize_f32", (
            self._ref("loss_ps"), nb, ws, 1.0 / (nb * feat) if mse_args is not None else 0.0, self._ref("loss_ce"),
            self._ref("loss_mse") if mse_args is not None else None, guard, step), tag="loss"))

    # ------------------------------------------------------------------ backward
    @staticmethod
    def _chanmap_start(ridx, cin):
        """Transpose of a monotone channel map: input channel ci receives output channels [start[ci], start[ci+1])."""
        ridx = np.asarray(ridx)
        assert (np.diff(ridx) >= 0).all(), "channel maps are monotone"
        return np.searchsorted(ridx, np.arange(cin + 1), side="left").astype(np.int32)

    def _foldable_residual(self, node):
        """Index of a shortcut of `node` whose gradient can ride in the epilogue of the node's own data-gradient
        GEMM: the shortcut source IS the convolution input (net = f(conv(net)) + map(net)), same pixel grid, plain
        (un-cropped) storage on both sides."""
        if node.kind != "conv" or not node.has_post:
            return None
        src = node.sources[0]
        if not self._needs_grad(src) or src.npix != node.out.npix:
            return None
        z_st = self.storage[id(node.out)]
        if z_st.pixmap is not None or z_st.ch_off != 0 or z_st.ld != node.cout:
            return None
        if not self.storage_of(src).contiguous:
            return None
        for k, (rsrc, _) in enumerate(node.residuals):
            if rsrc is src:
                return k
        return None

    def _bwd_residuals(self, node, dz_ref, lddz, rows, c, skip=None):
        for k, (src, ridx) in enumerate(node.residuals):
            if k == skip:
                continue
            if not self._needs_grad(src):
                continue
            gst, acc = self._grad_target(src)
            sref = None
            if ridx is not None:
                sref = self._upload(self._chanmap_start(ridx, src.c))
            self.bwd.append(Launch("chanmap_bwd", (dz_ref, lddz, rows, c, self._ref(gst.buf, gst.ch_off), gst.ld,
                                                   src.c, sref, acc), nbytes=4 * rows * (c + 2 * src.c),
                                   tag="res-bwd"))

    def _bwd_linear(self, idx, node):
        nb = self.nb
        out = node.out
        c = node.cout
        rows = out.npix * nb
        aux = self.node_aux[idx]
        own = out.owner
        if not self.grad_written.get(id(own), False):
            raise RuntimeError(f"node {idx} ({node.branches[0].scope}) receives no gradient")
        z_st = self.storage[id(out)]
        dz = self._ref("g:" + z_st.buf)
        y_ref = self._ref(aux["y"].buf)
        dy = dz  # backward post-op runs in place
        trains = self._trains([b.w for b in node.branches])
        fold = self._foldable_residual(node)
        fold_res = None
        if fold is not None:
            # the shortcut gradient is added by the data-gradient epilogue, which therefore needs dZ intact: the
            # post-op backward writes dY into its own buffer instead of over dZ
            ridx = node.residuals[fold][1]
            sref = None
            if ridx is not None:
                sref = self._upload(self._chanmap_start(ridx, node.sources[0].c))
            fold_res = (dz, c, sref)
            if node.has_bn or (node.act and node.act.code != 0) or aux.get("mask") is not None:
                self._alloc("dy:" + z_st.buf, rows * c)
                dy = self._ref("dy:" + z_st.buf)
        if node.has_post:
            self._bwd_residuals(node, dz, c, rows, c, skip=fold)
            self._emit_post_bwd(node, aux, dz, y_ref, rows, c, dy, want_param=trains)
        elif node.has_bias and trains:
            self._emit_post_bwd(node, aux, dz, y_ref, rows, c, None, want_param=True)

        # ---- data gradient ----
        if node.kind == "conv":
            src = node.sources[0]
            s_st = self.storage_of(src)
            h, w = src.hw
            if self._needs_grad(src):
                gst, acc = self._grad_target(src)
                by_cout = {}
                for b, col in self._columns(node):
                    by_cout.setdefault(b.cout, []).append((b, col))
                w_ref, w_ld, mtag = Ref(self.sess.params), None, ""
                lay = self._level_pass(idx, node, "dgrad")
                if lay is not None:  # one launch over the packed image
                    by_cout = {lay["co"]: self._columns(node)}
                    w_ref, w_ld, mtag = self._ref(lay["buf"]), lay["C"], "/merged"
                for cout, items in by_cout.items():
                    taps = self._taps(items, src.c, lay)
                    shape = GemmShape(n=src.c, lda=c, ta=0, ldb=w_ld or cout, tb=1, ldc=gst.ld)
                    tb = GemmTables()
                    per_pixel = []
                    if len(taps) == 1 and gst.contiguous:  # a lone 1x1 branch: ONE group over all pixels
                        _, _, w_, col, n = taps[0]
                        tb.add_group(gst.pix_off(0), [(col, w_, n)], src.npix * nb)
                    else:
                        # input pixel (iy, ix) sums one segment per tap: the tap's columns of dY at output pixel
                        # (iy - dy, ix - dx) -- merged level: 49 instead of 84 segments of 15 .. 60 columns at the centre
                        # of a 7x7 patch
                        wo, vr = self._valid_geometry(node)
                        ho, wo = (h, w) if wo is None else node.out.hw
                        per_pixel = [[(((iy - dy - vr) * wo + ix - dx - vr) * nb * c + col, w_, n)
                                      for dy, dx, w_, col, n in taps
                                      if 0 <= iy - dy - vr < ho and 0 <= ix - dx - vr < wo]
                                     for iy in range(h) for ix in range(w)]
                    # Segment splitting, the data-gradient twin of the forward tap splitting: an input pixel of a
                    # multi-kernel level sums up to sum(k^2) segments (165 for the five kernels of DUALCNN) and its
                    # block runs that much longer than a corner pixel's.  The segment list is cut into S chunks
                    # that write partial copies of dX (same layout, in scratch), processed chunk after chunk
                    # inside a row chunk, and a reduce adds them.  Not with a folded shortcut gradient (one epilogue).
                    max_segs = max(map(len, per_pixel), default=0)
                    S = 1
                    if (DGRAD_MAX_SEGS > 0 and fold_res is None and nb >= TAP_SPLIT_MIN_BATCH and gst.contiguous
                            and gst.ch_off == 0 and gst.ld == src.c and max_segs > DGRAD_MAX_SEGS):
                        S = -(-max_segs // DGRAD_MAX_SEGS)
                    if S > 1:
                        copy = h * w * nb * gst.ld
                        for pin, segs in enumerate(per_pixel):
                            for _, si, chunk in self._partial_copies(segs, S):
                                tb.add_group(si * copy + gst.pix_off(pin), chunk, nb, subkey=si)
                        pos = len(self.bwd)
                        self._emit_gemm(self.bwd, tb, shape, dy, w_ref, self._ref(gst.buf), None, 0,
                                        f"dgrad:{items[0][0].scope}/split{mtag}")
                        self._scratch(self.bwd[pos], "c", "scratch_dgrad", S * copy)
                        l2 = Launch("reduce_splits_f32", (None, copy, S, self._ref(gst.buf), h * w * nb * src.c,
                                                          acc, None, src.c, gst.ld),
                                    nbytes=4 * h * w * nb * src.c * (S + 1), tag="dgrad-split-reduce")
                        self._scratch(l2, "partial", "scratch_dgrad", S * copy)
                        self.bwd.append(l2)
                        acc = 1
                        continue
                    for pin, segs in enumerate(per_pixel):
                        tb.add_group(gst.pix_off(pin), segs, nb)
                    self._emit_gemm(self.bwd, tb, shape, dy, w_ref, self._ref(gst.buf), None, acc,
                                    f"dgrad:{items[0][0].scope}{mtag}", res=fold_res, pair=cout <= 16, kslice=True)
                    fold_res = None
                    acc = 1
            # ---- filter gradient ----
            if trains:
                self._wgrad_conv(idx, node, s_st, dy, c)
        elif node.kind == "blockdense":
            src = node.sources[0]
            s_st = self.storage_of(src)
            cout = node.branches[0].cout
            if self._needs_grad(src):
                gst, acc = self._grad_target(src)
                by_width = {}
                for pi, (off, width) in enumerate(node.in_slices):
                    by_width.setdefault(width, []).append((pi, off))
                for width, items in by_width.items():  # the last slice may be ragged: one launch per input width
                    tb = GemmTables()
                    for pi, off in items:
                        tb.add_group(gst.pix_off(0) + off, [(pi * cout, node.branches[pi].w.offset, cout)], nb)
                    self._emit_gemm(self.bwd, tb, GemmShape(n=width, lda=c, ta=0, ldb=cout, tb=1, ldc=gst.ld), dy,
                                    Ref(self.sess.params), self._ref(gst.buf), None, acc,
                                    f"dgrad:{node.branches[0].scope}+", allow_split=False)
            if trains:
                self._wgrad_blockdense(node, s_st, dy, c, cout)
        else:
            b = node.branches[0]
            rowbase = 0
            for src in node.sources:
                s_st = self.storage_of(src)
                if self._needs_grad(src):
                    gst, acc = self._grad_target(src)
                    tb = GemmTables()
                    for p in range(src.npix):
                        tb.add_group(gst.pix_off(p), [(0, b.w.offset + (rowbase + p * src.c) * c, c)], nb)
                    self._emit_gemm(self.bwd, tb, GemmShape(n=src.c, lda=c, ta=0, ldb=c, tb=1, ldc=gst.ld), dy,
                                    Ref(self.sess.params), self._ref(gst.buf), None, acc, f"dgrad:{b.scope}")
                rowbase += src.npix * src.c
            if trains:
                self._wgrad_dense(node, dy, c)

    def _emit_post_bwd(self, node, aux, dz, y_ref, rows, c, dy, want_param):
        has_bn = isinstance(node, G.LinearNode) and node.has_bn
        act = node.act
        code, alpha = (act.code, act.alpha) if act else (0, 0.0)
        mean = aux.get("mean") if has_bn else None
        rstd = aux.get("rstd") if has_bn else None
        beta = aux.get("beta_ref") if has_bn else None
        mask = aux.get("mask")
        dparam = None
        if want_param and isinstance(node, G.LinearNode):
            if has_bn:
                dparam = self._g(aux["beta"])
            elif node.has_bias:
                dparam = self._g(aux["bias"])
        if aux.get("small_bn") and has_bn and dy is not None:
            pacc = self._param_acc(aux["beta"]) if dparam is not None else 0
            self.bwd.append(Launch("bn_act_small_bwd", (dz, c, y_ref, c, rows, c, mean, rstd, beta, code, alpha, mask, c,
                                                        dy, c, dparam, pacc), nbytes=16 * rows * c,
                                   tag="post-bwd-small"))
            return
        sums = None
        if has_bn or dparam is not None:
            chunk = stat_chunk_rows(rows)
            n_chunks = (rows + chunk - 1) // chunk
            pacc = 0
            if dparam is not None:
                pacc = self._param_acc(aux["beta"] if has_bn else aux["bias"])
            if not has_bn and dy is not None and (code != 0 or mask is not None) and not self.sync_bn:
                # no batch norm: dY = dZ * act'(y) needs no column sum -- the bias-gradient reduction writes it too
                l1 = Launch("act_bias_bwd_reduce", (dz, c, y_ref, c, rows, c, code, alpha, mask, c, chunk, None, dy, c),
                            nbytes=12 * rows * c, tag="post-bwd-reduce+apply")
                if dparam is None:
                    # the phase does not train this layer: only dY is wanted, the chunk sums have no reader
                    self._scratch(l1, "partial", "scratch_partial", n_chunks * 2 * c)
                    self.bwd.append(l1)
                    return
                if self._defer_bias_sums:
                    # GAN train op: the chunk sums of every such layer stay in a buffer of their own and ONE launch at the end
                    # of the backward pass turns them all into bias gradients (PhasePlan._flush_slab_reduces)
                    k = self._bias_sum_bufs
                    self._bias_sum_bufs += 1
                    name = f"bias_sums:{k}"
                    self._alloc(name, n_chunks * 2 * c)
                    l1.set("partial", self._ref(name))
                    self.bwd.append(l1)
                    self._bias_sum_entries.append((self._ref(name), dparam, 2 * c, c, n_chunks, pacc))
                    return
                self._scratch(l1, "partial", "scratch_partial", n_chunks * 2 * c)
                l2 = Launch("bwd_reduce_finalize", (None, n_chunks, c, None, dparam, pacc), tag="post-bwd-finalize")
                self._scratch(l2, "partial", "scratch_partial", n_chunks * 2 * c)
                self._scratch(l2, "sums", "sums", 2 * c)
                self.bwd += [l1, l2]
                return
            else:
                l1 = Launch("bn_act_bwd_reduce", (dz, c, y_ref, c, rows, c, mean, rstd, beta, code, alpha, mask, c,
                                                  chunk, None), nbytes=8 * rows * c, tag="post-bwd-reduce")
                self._scratch(l1, "partial", "scratch_partial", n_chunks * 2 * c)
                l2 = Launch("bwd_reduce_finalize", (None, n_chunks, c, None, dparam, pacc), tag="post-bwd-finalize")
                self._scratch(l2, "partial", "scratch_partial", n_chunks * 2 * c)
                self._scratch(l2, "sums", "sums", 2 * c)
                self.bwd += [l1, l2]
            sums = "pending"
        sync = self.sync_bn and has_bn and node.training and sums is not None
        if sync:
            # sum(dyh), sum(dyh * xhat) over the GLOBAL batch (the parameter gradient above stays the local sum: it
            # travels in the flat gradient all-reduce)
            lc = Launch("_allreduce", (None, 2 * c), tag="bn-sync-reduce")
            self._scratch(lc, "ref", "sums", 2 * c)
            self.bwd.append(lc)
        if dy is not None and (has_bn or code != 0 or mask is not None):
            if sync:
                stat_rows = rows // self.nb * (self.global_nb if self.global_nb is not None else self.nb * self.world)
                l3 = Launch("bn_act_bwd_apply_global", (dz, c, y_ref, c, rows, c, mean, rstd, beta, code, alpha, mask, c,
                                                        None, int(stat_rows), dy, c), nbytes=12 * rows * c,
                            tag="post-bwd-apply")
            else:
                l3 = Launch("bn_act_bwd_apply", (dz, c, y_ref, c, rows, c, mean, rstd, beta, code, alpha, mask, c, None,
                                                 dy, c), nbytes=12 * rows * c, tag="post-bwd-apply")
            if sums is not None:
                self._scratch(l3, "sums", "sums", 2 * c)
            self.bwd.append(l3)

    def _emit_wgrad(self, groups, slab, w0_offset, n, a_ref, lda, b_ref, ldb, tag, acc=0, unpack=None):
        """Filter-gradient product: groups = [(c_off in the slab, [(a_off, b_off)] pixel pairs, rows, n or 0 = the launch's
        n)], each the sum over its pixel pairs and the batch rows; split s of the reduction (gemm_policy.wgrad_splits)
        writes its slab at s * slab.
        unpack (merged levels): dict(buf, entries) -- the product's output is a packed image in buffer `buf`, scattered into
        the gradient slots by block copies after the reduction."""
        s_pix, s_row = gemm_policy.wgrad_splits(sum((rows + GEMM_BM - 1) // GEMM_BM * (((gn or n) + 63) // 64)
                                                    for _, _, rows, gn in groups),
                                                max(len(prs) for _, prs, _, _ in groups), self.nb)
        S = s_pix * s_row
        tb = T.wgrad_split_tables(groups, self.nb, lda, ldb, slab, s_pix, s_row)
        if MERGE_WGRAD:
            if (acc or (unpack and any(e[6] for e in unpack["entries"]))) and self._pending_wgrads:
                # a second application of shared weights adds to what an earlier pending product writes: keep the order
                self._flush_wgrads()
            self._pending_wgrads.append(dict(tb=tb, S=S, slab=int(slab), w0=int(w0_offset), n=int(n), a_ref=a_ref,
                                             lda=int(lda), b_ref=b_ref, ldb=int(ldb), tag=tag, acc=int(acc), unpack=unpack))
            return
        assert unpack is None, "merged-level filter gradients need the merged launch (MERGE_WGRAD)"
        launch_pos = len(self.bwd)
        self._emit_gemm(self.bwd, tb, GemmShape(n=n, lda=lda, ta=1, ldb=ldb, tb=0, ldc=n), a_ref, b_ref,
                        Ref(self.sess.grads, w0_offset if S == 1 else 0), None, acc if S == 1 else 0, tag, allow_split=False)
        if S == 1:
            return
        l = self.bwd[launch_pos]
        self._scratch(l, "c", "scratch_wgrad", S * slab)
        l2 = Launch("reduce_splits_f32", (None, slab, S, Ref(self.sess.grads, w0_offset), slab, acc, None, 0, 0),
                    nbytes=4 * slab * (S + 1), tag="wgrad-reduce")
        self._scratch(l2, "partial", "scratch_wgrad", S * slab)
        self.bwd.append(l2)

    def _flush_wgrads(self):
        """Emit the collected filter gradients: one hypel_seg_gemm_multi_f32 per tile width over the blocks of every
        pending product (gemm_tables.merged_wgrad_tables: the XCD-laid record arrays), then one
        hypel_reduce_splits_multi_f32 that sums the split slabs into the gradient buffer and, for merged levels, the block
        copies that scatter the packed gradient images into the variables' gradient slots."""
        pend, self._pending_wgrads = self._pending_wgrads, []
        if not pend:
            return
        base = Ref(self.sess.params)
        rel = self._param_rel
        # scratch for the split slabs of this flush
        sname = f"wgrad_partials:{self._wgrad_flushes}"
        self._wgrad_flushes += 1
        self._alloc(sname, max(sum(e["S"] * e["slab"] for e in pend if e["S"] > 1), 1))
        grads0 = rel(Ref(self.sess.grads))
        for e in pend:
            n, tb, up = e["n"], e["tb"], e["unpack"]
            if up is not None:
                # the reduction target is the level's packed gradient image (dense per-offset blocks), scattered into the
                # variables' gradient slots afterwards
                self._alloc(up["buf"], e["slab"])
                e.update(out_base=rel(self._ref(up["buf"])), unpack=up["entries"])
            else:
                e["out_base"] = grads0 + e["w0"]
            e.update(a0=rel(e["a_ref"]), b0=rel(e["b_ref"]))
            sp6 = self._split6(e["tag"], tb, GemmShape(n=n, lda=e["lda"], ta=1, ldb=e["ldb"], tb=0, ldc=n), 0, False,
                               in_multi=True)
            # a merged level's per-offset products differ in their column count: each takes the width class of ITS n
            e["col_tiles"] = [gemm_policy.col_tiles(gn, sp6 if gn == n else gemm_policy.split6_width(gn)
                                                    if sp6 and gn > gemm_policy.GEMM_SPLIT_MIN_N else 0)
                              for gn in (tb.n_of(gi, n) for gi in range(len(tb.groups)))]
        launches, entries, unpacks = T.merged_wgrad_tables(pend, grads0, rel(self._ref(sname)))
        for m in launches:
            width = m["width"]
            s_r, r_r = self._upload(m["segs"]), self._upload(m["records"])
            l = Launch("seg_gemm_multi_f32", (base, 1, 0, width, s_r, r_r, int(len(m["records"]))),
                       flops=2 * m["macs"], nbytes=m["nbytes"],
                       tag=f"wgrad-merged/{'s' if width & GEMM_MULTI_SPLIT6 else ''}{width & 0xff}")
            l.meta = {"products": m["tags"], "blocks": m["blocks"], "xcd_work": m["xcd_work"]}
            self.bwd.append(l)
        if entries:
            e_r = self._upload(np.array(entries, REDUCE_ENTRY_DTYPE))
            l = Launch("reduce_splits_multi_f32", (base, e_r, len(entries)),
                       nbytes=4 * sum(cnt * (S + 1) for (_, _, _, cnt, S, _) in entries), tag="wgrad-reduce")
            l.meta = {"splits": [int(S) for (_, _, _, _, S, _) in entries]}
            self.bwd.append(l)
        if unpacks:
            u_r = self._upload(np.array(unpacks, COPY_BLOCK_DTYPE))
            self.bwd.append(Launch("copy_blocks_f32", (base, u_r, len(unpacks), max(u[2] * u[3] for u in unpacks)),
                                   nbytes=8 * sum(u[2] * u[3] for u in unpacks), tag="level-unpack"))

    def _wgrad_conv(self, idx, node, s_st, dy_ref, c):
        """Filter gradient of a convolution: per tap ONE product dW[tap] = sum_p X[p + (dy, dx)]^T dY[p][:, col:col + n] over
        the output pixels p whose input pixel is real.  A merged level: per input offset d, n = C - col0[ring] columns (30 ..
        120 for the 30-filter HYPELCNN level instead of 30 per (branch, tap)) into a dense packed image, whose [Cin x cout]
        slices hypel_copy_blocks_f32 scatters into the HWIO gradient slots."""
        nb = self.nb
        src = node.sources[0]
        h, w = src.hw

        wo, vr = self._valid_geometry(node)
        ho, wo = (h, w) if wo is None else node.out.hw

        def pairs(dy, dx, col):
            return [(s_st.pix_off((oy + vr + dy) * w + ox + vr + dx), (oy * wo + ox) * nb * c + col)
                    for oy in range(ho) for ox in range(wo) if 0 <= oy + vr + dy < h and 0 <= ox + vr + dx < w]

        lay = self._level_pass(idx, node, "wgrad")
        # (every offset of the largest kernel must meet at least one pixel pair, or its block of the packed image would
        # never be written: (k - 1) / 2 <= min(h, w) - 1)
        if lay is not None and max(b.k for b in node.branches) <= 2 * min(h, w) - 1:
            taps = self._taps(self._columns(node), src.c, lay)
            ents = []
            for b, col in self._columns(node):
                acc = self._param_acc(b.w)
                for dy, dx, w_, _, _ in self._taps([(b, col)], src.c):
                    d = lay["index"][(dy, dx)]
                    _, _, _, col0, n_d = taps[d]
                    ents.append((lay["dense_off"][d] + col - col0, w_, src.c, b.cout, n_d, b.cout, acc))
            self._emit_wgrad([(lay["dense_off"][d], pairs(dy, dx, col), src.c, n_d) for d, (dy, dx, _, col, n_d) in enumerate(taps)],
                             lay["dense_size"], 0, lay["C"], self._ref(s_st.buf), s_st.ld, dy_ref, c,
                             f"wgrad:{node.branches[0].scope}/merged", unpack=dict(buf=f"dwpack:{idx}", entries=ents))
            return
        by_cout = {}
        for b, col in self._columns(node):
            by_cout.setdefault(b.cout, []).append((b, col))
        for cout, items in by_cout.items():
            # the slab of one launch = the contiguous weights of its branches
            lo = min(b.w.offset for b, _ in items)
            slab = max(b.w.offset + b.w.size for b, _ in items) - lo
            if slab != sum(b.w.size for b, _ in items):
                # the reduce overwrites the whole slab: sibling branches of another width in between would be clobbered
                raise RuntimeError(f"filter-gradient slab of {items[0][0].scope}: branches with {cout} filters are not "
                                   f"contiguous in the parameter buffer")
            acc = max(self._param_acc(b.w) for b, _ in items)
            self._emit_wgrad([(w_ - lo, pairs(dy, dx, col), src.c, 0) for dy, dx, w_, col, _ in self._taps(items, src.c)],
                             slab, lo, cout, self._ref(s_st.buf), s_st.ld, dy_ref, c, f"wgrad:{items[0][0].scope}", acc=acc)

    def _wgrad_dense(self, node, dy, c):
        """One product per source; a group per source pixel: its block of weight rows, one pixel pair."""
        b = node.branches[0]
        rowbase = 0
        for src in node.sources:
            s_st = self.storage_of(src)
            acc = self._param_acc(b.w) if rowbase == 0 else (1 if b.w.name + f"#{rowbase}" in self.param_written else 0)
            self.param_written.add(b.w.name + f"#{rowbase}")
            self._emit_wgrad([(p * src.c * c, [(s_st.pix_off(p), 0)], src.c, 0) for p in range(src.npix)],
                             src.npix * src.c * c, b.w.offset + rowbase * c, c, self._ref(s_st.buf), s_st.ld, dy, c,
                             f"wgrad:{b.scope}", acc=acc)
            rowbase += src.npix * src.c

    def _wgrad_blockdense(self, node, s_st, dy, c, cout):
        """dW_p = X[:, slice_p]^T dY[:, p*cout:(p+1)*cout] for every slice p in one launch (the weights of a merged
        layer are contiguous: one slab per batch-row split, one reduction)."""
        ws = [b.w for b in node.branches]
        lo = ws[0].offset
        acc = self._param_acc(ws[0])
        for w in ws[1:]:
            self.param_written.add(w.name)
        self._emit_wgrad([(w.offset - lo, [(s_st.pix_off(0) + off, pi * cout)], width, 0)
                          for pi, (w, (off, width)) in enumerate(zip(ws, node.in_slices))],
                         sum(w.size for w in ws), lo, cout, self._ref(s_st.buf), s_st.ld, dy, c,
                         f"wgrad:{node.branches[0].scope}+", acc=acc)

    def _bwd_post(self, idx, node):
        out, src = node.out, node.src
        rows, c = out.npix * self.nb, out.c
        aux = self.node_aux[idx]
        z_st = self.storage[id(out)]
        if not self.grad_written.get(id(out.owner), False):
            raise RuntimeError(f"post node {idx} receives no gradient")
        dz = self._ref("g:" + z_st.buf)
        self._bwd_residuals(node, dz, c, rows, c)
        if not self._needs_grad(src):
            return
        s_st = self.storage_of(src)
        act = node.act
        code, alpha = (act.code, act.alpha) if act else (0, 0.0)
        mask = aux.get("mask")
        if code != 0 or mask is not None:
            self.bwd.append(Launch("bn_act_bwd_apply", (dz, c, self._ref(s_st.buf, s_st.ch_off), s_st.ld, rows, c, None,
                                                        None, None, code, alpha, mask, c, None, dz, c),
                                   nbytes=12 * rows * c, tag="post-bwd-apply"))
        gst, acc = self._grad_target(src)
        self.bwd.append(Launch("chanmap_bwd", (dz, c, rows, c, self._ref(gst.buf, gst.ch_off), gst.ld, c, None, acc),
                               nbytes=12 * rows * c, tag="post-bwd-pass"))

    def _bwd_lrn(self, idx, node):
        out, src = node.out, node.src
        rows, c = out.npix * self.nb, out.c
        z_st = self.storage[id(out)]
        if not self.grad_written.get(id(out.owner), False):
            raise RuntimeError(f"lrn node {idx} receives no gradient")
        if not self._needs_grad(src):
            return
        s_st = self.storage_of(src)
        gst, acc = self._grad_target(src)
        self.bwd.append(Launch("lrn_bwd", (self._ref(s_st.buf, s_st.ch_off), s_st.ld, self._ref("g:" + z_st.buf), c,
                                           rows, c, node.radius, float(node.bias), float(node.alpha), float(node.beta),
                                           self._ref(gst.buf, gst.ch_off), gst.ld, acc), nbytes=16 * rows * c,
                               tag="lrn-bwd"))

    # ------------------------------------------------------------------ capsules (csrc/capsule.hip)
    def _fwd_capsule(self, idx, node):
        """Prediction vectors u_hat [N, I, J*D] (one pass that reads every W_i once), then per routing iteration one
        launch that sums over the capsules (s_r, squash -> v_r) and one that sums the agreement over the batch
        (b_{r+1}, softmax -> c_{r+1}); the last iteration writes y_conv instead.  Kept for the backward pass: u_hat,
        every c_r, s_r and v_r.  Coefficients live in ONE buffer [2R-1][I][J] (c_0 .. c_{R-1}, then the backward pass's
        db_1 .. db_{R-1}) and the batch vectors in ONE buffer [2R-1][N][J*D] (the backward pass's ds_0 .. ds_{R-1}, then
        v_0 .. v_{R-2}): the gradient of u_hat is the sum of their 2R-1 outer products and is never written to memory."""
        if getattr(self.sess, "dist", None) is not None:
            raise NotImplementedError("capsule routing is single-device only: its agreement is summed over the batch, so "
                                      "data parallel (WORLD_SIZE > 1) would need an all-reduce inside every routing iteration")
        nb, src = self.nb, node.src
        if nb > G.CAPSULE_MAX_BATCH:
            raise NotImplementedError(f"capsule routing: a batch of {nb} exceeds the {G.CAPSULE_MAX_BATCH} samples one launch of "
                                      "the routing kernels covers (the sample index is a grid dimension): use a smaller "
                                      "batch size")
        J, D, R, I = node.classes, node.width, node.iterations, node.capsules
        M = src.c // D
        jd = J * D
        s_st = self.storage_of(src)
        self._assert_contiguous(node.weights)
        self._assert_contiguous(node.biases)
        aux = {"x": s_st, "pix": self._upload(np.asarray([s_st.pix_off(p) for p in range(src.npix)], np.int64))}
        self.node_aux[idx] = aux
        self._alloc(f"uhat:{idx}", nb * I * jd)
        self._alloc(f"capc:{idx}", (2 * R - 1) * I * J)
        import torch
        self._alloc(f"capb:{idx}", max(R - 1, 1) * I * J, torch.float64)  # routing logits: fp64 (they grow with the batch)
        self._alloc(f"capvec:{idx}", (2 * R - 1) * nb * jd)
        self._alloc(f"caps:{idx}", R * nb * jd)
        y_st = self._new_value(node.out, f"capy:{idx}")
        v_st = self._new_value(node.out_v, f"capv:{idx}")
        uhat, cc, vec = self._ref(f"uhat:{idx}"), self._ref(f"capc:{idx}"), self._ref(f"capvec:{idx}")
        ubytes = 4 * nb * I * jd
        self.fwd.append(Launch("caps_uhat_fwd", (self._ref(s_st.buf), aux["pix"], s_st.ld, M, self._p(node.weights[0]),
                                                 self._p(node.biases[0]), nb, I, D, jd, uhat),
                               nbytes=ubytes + 4 * I * (D + 1) * jd, tag="caps-uhat"))
        self.fwd.append(Launch("fill_f32", (cc, I * J, 1.0 / J), tag="caps-c0"))
        for r in range(R):
            last = r == R - 1
            v_ref = self._ref(v_st.buf) if last else vec + (R + r) * nb * jd
            self.fwd.append(Launch("caps_route_fwd", (uhat, cc + r * I * J, nb, I, J, D,
                                                      self._ref(f"caps:{idx}", r * nb * jd), v_ref,
                                                      self._ref(y_st.buf) if last else None), nbytes=ubytes,
                                   tag="caps-route"))
            if not last:
                self.fwd.append(Launch("caps_agree_fwd", (uhat, v_ref, nb, I, J, D,
                                                          self._ref(f"capb:{idx}", (r - 1) * I * J) if r > 0 else None,
                                                          self._ref(f"capb:{idx}", r * I * J), cc + (r + 1) * I * J),
                                       nbytes=ubytes, tag="caps-agree"))

    def _bwd_capsule(self, idx, node):
        """Reverse sweep over the routing iterations: ds_{R-1} from the gradients of y_conv and v; then for r = R-1 .. 1
        one pass over u_hat for dc_r (-> db_r through the softmax) and one for dv_{r-1} (-> ds_{r-1} through the squash);
        c_0 is a constant, so iteration 0 reads nothing.  One last launch builds du_hat on the fly from the 2R-1
        (coefficient, batch vector) pairs and reduces it into dW_i, dbias_i and dx."""
        nb, src = self.nb, node.src
        J, D, R, I = node.classes, node.width, node.iterations, node.capsules
        M = src.c // D
        jd = J * D
        aux = self.node_aux[idx]
        s_st = aux["x"]
        y_st, v_st = self.storage[id(node.out)], self.storage[id(node.out_v)]
        gy = self._ref("g:" + y_st.buf) if self.grad_written.get(id(node.out), False) else None
        gv = self._ref("g:" + v_st.buf) if self.grad_written.get(id(node.out_v), False) else None
        if gy is None and gv is None:
            raise RuntimeError(f"capsule node {idx} receives no gradient")
        uhat, cc, vec = self._ref(f"uhat:{idx}"), self._ref(f"capc:{idx}"), self._ref(f"capvec:{idx}")
        ss = self._ref(f"caps:{idx}")
        ubytes = 4 * nb * I * jd
        self.bwd.append(Launch("caps_head_bwd", (gy, gv, ss + (R - 1) * nb * jd, nb, J, D, vec + (R - 1) * nb * jd),
                               tag="caps-head-bwd"))
        for r in range(R - 1, 0, -1):
            db = cc + (R + r - 1) * I * J
            self.bwd.append(Launch("caps_agree_bwd", (uhat, vec + r * nb * jd, nb, I, J, D, cc + r * I * J,
                                                      cc + (R + r) * I * J if r < R - 1 else None, db),
                                   nbytes=ubytes, tag="caps-agree-bwd"))
            self.bwd.append(Launch("caps_route_bwd", (uhat, db, nb, I, J, D, ss + (r - 1) * nb * jd,
                                                      vec + (r - 1) * nb * jd), nbytes=ubytes, tag="caps-route-bwd"))
        trains = self._trains(node.weights)
        dw = db_ = None
        acc_w = 0
        if trains:
            dw, db_ = self._g(node.weights[0]), self._g(node.biases[0])
            acc_w = max([self._param_acc(v) for v in node.weights + node.biases])
        dx, lddx, acc_x, dpix = None, 0, 0, aux["pix"]
        if self._needs_grad(src):
            gst, acc_x = self._grad_target(src)
            dx, lddx = self._ref(gst.buf), gst.ld
            if [gst.pix_off(p) for p in range(src.npix)] != [s_st.pix_off(p) for p in range(src.npix)]:
                dpix = self._upload(np.asarray([gst.pix_off(p) for p in range(src.npix)], np.int64))
        self.bwd.append(Launch("caps_uhat_bwd", (self._ref(s_st.buf), aux["pix"], s_st.ld, M, self._p(node.weights[0]), nb,
                                                 I, J, D, 2 * R - 1, cc, vec, dw, db_, acc_w, dx, dpix, lddx, acc_x),
                               nbytes=4 * I * (D + 1) * jd * (2 if trains else 1), tag="caps-uhat-bwd"))

    def _fwd_label_mask(self, idx, node):
        v_st, l_st = self.storage_of(node.src), self.storage_of(node.labels)
        st = self._new_value(node.out, f"z:{idx}")
        self.fwd.append(Launch("caps_mask_fwd", (self._ref(v_st.buf, v_st.ch_off), v_st.ld, self._ref(l_st.buf, l_st.ch_off),
                                                 l_st.ld, self.nb, node.classes, node.width, self._ref(st.buf), st.ld),
                               tag="caps-mask"))

    def _bwd_label_mask(self, idx, node):
        z_st = self.storage[id(node.out)]
        if not self.grad_written.get(id(node.out.owner), False):
            raise RuntimeError(f"label mask node {idx} receives no gradient")
        if not self._needs_grad(node.src):
            return
        l_st = self.storage_of(node.labels)
        gst, acc = self._grad_target(node.src)
        self.bwd.append(Launch("caps_mask_bwd", (self._ref("g:" + z_st.buf), z_st.ld, self._ref(l_st.buf, l_st.ch_off),
                                                 l_st.ld, self.nb, node.classes, node.width, self._ref(gst.buf, gst.ch_off),
                                                 gst.ld, acc), tag="caps-mask-bwd"))


# =========================================================================================== GAN phases
