"""One digest per planner configuration: the check that a host-side refactor of the planner leaves every plan as it was.

    python tools/plan_digest.py [ROOT] [--only SUBSTRING] [--dump DIR] > digests.txt

ROOT = the checkout whose hypelcnn_amd / tests / oracle are imported (default: the one this file lies in), so the same
script digests two trees; diff the two outputs.  Plans are built on the test emulation (tests/emu_backend.py), no GPU.

A digest covers every plan a configuration builds, in construction order: buffer names and sizes, scratch sizes, sync
points, and for every launch of fwd and bwd, in order: name, tag, flops, bytes, kparts, meta, every scalar argument,
every Ref argument as (buffer name or session array, element offset) and, for an uploaded table, a hash of its bytes.
Tables hold element distances between buffers (TowerPlan._param_rel), so buffers come from one arena in allocation order:
the distances then depend on the sequence of allocations alone.  --dump DIR writes the digested text per configuration.

Configurations: the four bench.py workloads at their benchmark batch and at batch 64 (training and inference towers, every
GAN train op and its pool generator); the data-parallel plans of tests/test_dp_gloo.py (rank 0 of two ranks: planning
issues no collective, so the session's `dist` is set directly), sync-BN off and on; every case of
tests/test_host_plan_emu.py and tests/test_gan_emu.py that builds a plan, with its patched constants.
"""
import argparse
import hashlib
import importlib
import json
import mmap
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ARENA_BYTES = 1 << 40  # address space only: pages are committed when written


def make_backend():
    from tests.emu_backend import EmuBackend

    class ArenaBackend(EmuBackend):
        """Buffers are consecutive 256-byte aligned slices of one lazily committed mapping."""

        def __init__(self):
            super().__init__()
            flags = mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, "MAP_NORESERVE", 0x4000)
            self._map = mmap.mmap(-1, ARENA_BYTES, flags=flags)
            self._arena = torch.frombuffer(self._map, dtype=torch.uint8)
            self._pos = 0

        def zeros(self, n, dtype=torch.float32):
            nbytes = int(n) * torch.empty(0, dtype=dtype).element_size()
            t = self._arena[self._pos:self._pos + nbytes].view(dtype)
            self._pos += (nbytes + 255) // 256 * 256
            return t

        empty = zeros

    return ArenaBackend()


class Patches:
    """setattr on whichever planner module owns the constant, undone on exit."""

    MODULES = ("hypelcnn_amd.plan", "hypelcnn_amd.gemm_policy")

    def __init__(self, values):
        self.values, self.undo = values, []

    def __enter__(self):
        mods = []
        for m in self.MODULES:
            try:
                mods.append(importlib.import_module(m))
            except ImportError:
                pass
        for name, value in self.values.items():
            owners = [m for m in mods if hasattr(m, name)]
            if not owners:
                raise KeyError(name)
            # (flag bits may be re-exported; a tunable has one home -- take the last module that has it: the policy)
            self.undo.append((owners[-1], name, getattr(owners[-1], name)))
            setattr(owners[-1], name, value)

    def __exit__(self, *exc):
        for mod, name, old in reversed(self.undo):
            setattr(mod, name, old)


def describe(plans):
    """The digested text of the plans one configuration built."""
    lines = []
    for k, plan in enumerate(plans):
        sess = plan.sess
        names = {}
        for attr in ("params", "grads", "state", "slot_m", "slot_v"):
            t = getattr(sess, attr, None)
            if t is not None:
                names[id(t)] = "sess." + attr
        for key, t in getattr(sess, "shared_inputs", {}).items():
            names[id(t)] = f"shared:{key}"
        for name, t in plan.buffers.items():
            names.setdefault(id(t), name)
        tables = {id(t): t for t in plan.tables}
        spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), n_, t)
                       for n_, t in [(names[id(t)], t) for t in list(plan.buffers.values())
                                     + [getattr(sess, a) for a in ("params", "grads", "state", "slot_m", "slot_v")
                                        if getattr(sess, a, None) is not None]])

        def ref(r):
            t = r.t
            if id(t) in tables:
                h = hashlib.sha256(t.numpy().tobytes()).hexdigest()[:16]
                return f"table[{t.numel()}x{t.element_size()}:{h}]+{r.off}"
            if id(t) in names:
                return f"{names[id(t)]}+{r.off}"
            p = r.ptr()
            for lo, hi, n_, bt in spans:  # a view of a known buffer
                if lo <= p < hi:
                    return f"{n_}@{(p - lo) // bt.element_size()}"
            return f"?[{t.numel()}]+{r.off}"

        def arg(a):
            if a is None or isinstance(a, (bool, int, str)):
                return repr(a)
            if isinstance(a, float):
                return float(a).hex()
            if isinstance(a, (np.integer, np.floating)):
                return repr(a.item())
            if hasattr(a, "t") and hasattr(a, "off"):
                return ref(a)
            return f"<{type(a).__name__}>"

        lines.append(f"== plan {k}: {type(plan).__name__} nb={plan.nb} training={plan.training} "
                     f"sync_bn={getattr(plan, 'sync_bn', None)} global_nb={getattr(plan, 'global_nb', None)}")
        lines.append("buffers " + " ".join(f"{n_}:{t.numel()}:{t.dtype}" for n_, t in plan.buffers.items()))
        lines.append("scratch " + json.dumps(plan.scratch_sizes, sort_keys=True))
        lines.append("sync_points " + repr([tuple(int(v) for v in p) for p in plan.sync_points]))
        for lname, lst in (("fwd", plan.fwd), ("bwd", plan.bwd)):
            for i, l in enumerate(lst):
                lines.append(f"{lname}[{i}] {l.name} tag={l.tag!r} flops={int(l.flops)} bytes={int(l.bytes)} "
                             f"kparts={l.kparts} meta={json.dumps(l.meta, sort_keys=True, default=str)} "
                             f"args=({', '.join(arg(a) for a in l.args)})")
    return "\n".join(lines) + "\n"


# ---------------------------------------------------------------------------------------------------- configurations
ALG_H = {"drop_out_ratio": 0.7, "filter_count": 48, "learning_rate": 3e-4, "learning_rate_decay_factor": 0.96,
         "learning_rate_decay_step": 350, "lrelu_alpha": 0.18, "optimizer": "AdamOptimizer", "bn_decay": 0.95,
         "l2regularizer_scale": 1e-5, "spectral_hierarchy_level": 3, "spatial_hierarchy_level": 3,
         "degradation_coeff": 3, "use_residual": True, "batch_size": 6}
ALG_D = {"drop_out_ratio": 0.7, "lrelu_alpha": 0.18, "filter_count": 32, "hs_lidar_diff": 1,
         "optimizer": "AdamOptimizer", "learning_rate": 3e-4, "learning_rate_decay_factor": 0.96,
         "learning_rate_decay_step": 350}
ALG_C = {"drop_out_ratio": 0.5, "filter_count": 6, "optimizer": ["MomentumOptimizer", 0.9], "learning_rate": 1e-3,
         "learning_rate_decay_factor": 0.01, "learning_rate_decay_step": 33333}
ALG_DP = dict(ALG_H, spectral_hierarchy_level=2, spatial_hierarchy_level=2)
ALG_DP.pop("batch_size")
ALG_DUAL_DP = {"drop_out_ratio": 0.7, "filter_count": 96, "learning_rate": 3e-4, "learning_rate_decay_factor": 0.96,
               "learning_rate_decay_step": 350, "lrelu_alpha": 0.18, "optimizer": "AdamOptimizer", "bn_decay": 0.95,
               "l2regularizer_scale": 1e-5, "hs_lidar_diff": 1}
BENCH_CLASSIFIERS = {"hypelcnn": ("HYPELCNNModel", "alg_param_hypelcnn.json", 7, 145, 15, 1024),
                     "dualcnn": ("DUALCNNModel", "alg_param_dualcnn.json", 11, 49, 20, 512)}
BENCH_GANS = {"cyclegan": ("cycle_gan", 64, 2048), "cut": ("cut_x2y", 360, 4096)}


def classifier(model, patch, ch, classes, alg, nb, external_masks=True, with_eval=False, dist=None, sync_bn=False,
               global_nb=None):
    def run(root):
        from tests import parity_util as U
        built = U.build(model, patch, ch, classes, alg, make_backend(), with_eval=with_eval)
        built.ctx.external_masks = external_masks
        sess = built.ctx.session()
        if dist is not None:
            sess.dist = dist
        ct = sess.compile(built.train_tower, nb, loss=built.train_step.loss, external_masks=external_masks,
                          global_nb=global_nb, sync_bn=sync_bn)
        if with_eval:
            sess.compile(built.eval_tower, nb)
        return ct
    return run


def bench_classifier(workload, nb, dist=None):
    name, cfg, patch, ch, classes, _ = BENCH_CLASSIFIERS[workload]

    def run(root):
        alg = json.load(open(os.path.join(root, "hypelcnn_amd", "nnmodel", "modelconfigs", cfg)))
        alg["batch_size"] = nb
        return classifier(name, patch, ch, classes, alg, nb, external_masks=False, with_eval=True, dist=dist)(root)
    return run


def gan_phases(ops, sess, n):
    for phase in ops.loss.phases:
        ops._compiled(sess, phase, n)
        if phase.pool:
            sess.compile_phase(ops.loss.tower, n, outputs=[t for _, t in phase.pool], key="generate")


def bench_gan(workload, nb):
    kind, bands, _ = BENCH_GANS[workload]

    def run(root):
        from hypelcnn_amd.gan.wrapper_registry import get_wrapper_dict
        from hypelcnn_amd.gan.wrappers import gan_common as C
        flags = SimpleNamespace(discriminator_reg_scale=1e-5, gen_disc_reg_scale=1e-4, embedded_feat_size=2, patches=6,
                                cycle_consistency_loss_weight=10.0, identity_loss_weight=0.5, use_identity_loss=True,
                                nce_loss_weight=10.0, tau=0.07, batch_size=nb)
        wrapper = get_wrapper_dict(flags)[kind]
        wrapper.backend = make_backend()
        tower, xs, ys = C.new_gan_tower(bands)
        model = wrapper.define_model(xs, ys)
        loss = wrapper.define_loss(model)
        ops = wrapper.define_train_ops(model, loss, max_number_of_steps=100000, generator_lr=2e-4,
                                       discriminator_lr=1e-4, gen_discriminator_lr=1e-4)
        gan_phases(ops, ops.ctx.session(), nb)
    return run


def test_gan(kind, bands, patches, n=6):
    def run(root):
        from oracle import gan as OG
        from tests import gan_util as GU
        cfg = OG.GanConfig(kind, bands, patches=patches, max_steps=20)
        wrapper, model, loss, ops = GU.build(cfg, n, make_backend())
        gan_phases(ops, ops.ctx.session(), n)
    return run


def twice_applied(root):
    from tests import gan_util as GU
    GU.TwiceAppliedLayer(make_backend())


def configurations():
    """[(name, {constant: value}, run(root))]"""
    H, D, C = "HYPELCNNModel", "DUALCNNModel", "CONCNNModel"
    out = []
    for w, (_, _, _, _, _, dflt) in BENCH_CLASSIFIERS.items():
        for nb in (dflt, 64):
            out.append((f"bench/{w}/nb{nb}", {}, bench_classifier(w, nb)))
    for w, (_, _, dflt) in BENCH_GANS.items():
        for nb in (dflt, 64):
            out.append((f"bench/{w}/nb{nb}", {}, bench_gan(w, nb)))
    # data parallel (tests/test_dp_gloo.py: _worker, _syncbn_worker, _dual_worker) + the headline on eight ranks
    for sbn in (False, True):
        out.append((f"dp/hypelcnn-toy/nb4/syncbn{int(sbn)}", {},
                    classifier(H, 5, 9, 4, ALG_DP, 4, dist=(2, 0), sync_bn=sbn, global_nb=8)))
        out.append((f"dp/hypelcnn-toy/nb3of5/syncbn{int(sbn)}", {},
                    classifier(H, 5, 9, 4, ALG_DP, 3, dist=(2, 0), sync_bn=sbn, global_nb=5)))
    out.append(("dp/dualcnn-toy/buckets", {"DP_TWO_BUCKET_BYTES": 0, "DP_BUCKET_BYTES": 64 << 10},
                classifier(D, 7, 9, 4, ALG_DUAL_DP, 2, dist=(2, 0))))
    out.append(("dp/bench-hypelcnn/nb1024/world8", {}, bench_classifier("hypelcnn", 1024, dist=(8, 0))))
    # tests/test_host_plan_emu.py
    for i, (m, p, ch, cl, alg, nb) in enumerate([(H, 5, 11, 4, ALG_H, 6), (H, 7, 9, 4, dict(ALG_H, filter_count=96), 5),
                                                 (H, 3, 7, 3, dict(ALG_H, use_residual=False, spectral_hierarchy_level=2), 5),
                                                 (D, 5, 7, 3, ALG_D, 4), (C, 5, 9, 3, ALG_C, 4)]):
        out.append((f"emu/train_step/{i}", {}, classifier(m, p, ch, cl, alg, nb, with_eval=True)))
    tap = {"TAP_SPLIT_MIN_BATCH": 1, "MAX_TAPS_PER_TILE": 4}
    out.append(("emu/tap_split", tap, classifier(H, 7, 9, 4, ALG_H, 5)))
    out.append(("emu/biased_tap_channel_part", dict(tap, L2_CHUNK_BYTES=4096), classifier(D, 5, 7, 3, ALG_D, 4)))
    out.append(("emu/channel_part_bn", dict(tap, L2_CHUNK_BYTES=4096),
                classifier(H, 5, 9, 4, dict(ALG_H, filter_count=96), 5)))
    sp6 = {"GEMM_SPLIT": 6, "GEMM_SPLIT_MIN_FLOPS": 0.0}
    out.append(("emu/split6", sp6, classifier(H, 5, 40, 4, dict(ALG_H, filter_count=96), 70)))
    for merged in (False, True):
        pt = {"TAP_SPLIT_MIN_BATCH": 1, "DGRAD_MAX_SEGS": 5}
        if not merged:
            pt["MERGE_LEVELS"] = set()
        out.append((f"emu/dgrad_segment_split/merged{int(merged)}", pt, classifier(D, 5, 7, 3, ALG_D, 4)))
    out.append(("emu/wgrad_row_ranges/dualcnn", {"TARGET_BLOCKS": 1}, classifier(D, 5, 7, 3, ALG_D, 192)))
    out.append(("emu/wgrad_row_ranges/hypelcnn", {"TARGET_BLOCKS": 1}, classifier(H, 5, 11, 4, ALG_H, 192)))
    out.append(("emu/all_large_batch", {"MAX_TAPS_PER_TILE": 4, "DGRAD_MAX_SEGS": 5, "L2_CHUNK_BYTES": 1 << 16,
                                        "TARGET_BLOCKS": 4}, classifier(D, 5, 7, 3, ALG_D, 64)))
    out.append(("emu/unmerged_wgrad", {"MERGE_WGRAD": False}, classifier(H, 7, 9, 4, dict(ALG_H, filter_count=96), 5)))
    for passes, patch, fc in [("fwd", 7, 48), ("fwd,dgrad", 7, 48), ("fwd,dgrad", 5, 96), ("dgrad", 5, 48), ("wgrad", 7, 96),
                              ("fwd,dgrad,wgrad", 5, 480), ("fwd,dgrad,wgrad", 7, 48)]:
        pt = {"TAP_SPLIT_MIN_BATCH": 1, "MAX_TAPS_PER_TILE": 5, "MERGE_LEVELS": set(passes.split(",")),
              "MERGE_LEVELS_MAX_COUT": 1 << 20, "MERGE_WGRAD_MIN_COUT": 1, "MERGE_WGRAD_MAX_COUT": 1 << 20,
              "MERGE_SPLIT_KPARTS": True}
        if patch == 5:
            pt["L2_CHUNK_BYTES"] = 4096
        out.append((f"emu/merged_levels/{passes}/p{patch}/fc{fc}", pt,
                    classifier(H, patch, 9, 4, dict(ALG_H, filter_count=fc), 5)))
    out.append(("emu/merged_forward_split_off",
                {"TAP_SPLIT_MIN_BATCH": 1, "MAX_TAPS_PER_TILE": 5, "L2_CHUNK_BYTES": 4096,
                 "SPLIT_OVERRIDE": {"fwd:connector_0_conv1x1/merged": 0}},
                classifier(H, 7, 9, 4, dict(ALG_H, filter_count=192), 5)))
    for frac in (0.25, 0.75):
        pt = dict(sp6, KSLICE_MIN_GAIN=-10.0, KSLICE_MIN_K=4, KSLICE_OVERHEAD_K=1, KSLICE_REDUCE_COST_K=0,
                  KSLICE_FRAC_MIN=frac, KSLICE_SLOTS={1: 8, 2: 8, 3: 8})
        out.append((f"emu/kslice/frac{frac}", pt, classifier(H, 5, 40, 4, dict(ALG_H, filter_count=400), 150)))
    # tests/test_gan_emu.py
    for kind, bands, patches in [("cycle_gan", 16, 4), ("gan_x2y", 16, 4), ("gan_y2x", 24, 4), ("cut_x2y", 24, 6),
                                 ("cut_y2x", 64, 6), ("dcl_gan", 16, 4), ("dcl_cycle_gan", 16, 4)]:
        out.append((f"gan_emu/{kind}/b{bands}", {}, test_gan(kind, bands, patches)))
    out.append(("gan_emu/twice_applied_layer", {}, twice_applied))
    for fused in (True, False):
        out.append((f"gan_emu/act_in_gemm{int(fused)}", {"ACT_IN_GEMM": fused}, test_gan("cut_x2y", 144, 6)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("root", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--only", default="", help="run the configurations whose name contains this")
    ap.add_argument("--dump", default=None, metavar="DIR", help="write the digested text of every configuration here")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    from hypelcnn_amd import plan as P
    assert os.path.abspath(P.__file__).startswith(root + os.sep), P.__file__
    built = []
    init = P.TowerPlan.__init__

    def recording_init(self, *a, **kw):
        init(self, *a, **kw)
        built.append(self)

    P.TowerPlan.__init__ = recording_init
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    configs = [c for c in configurations() if args.only in c[0]]
    for name, patches, run in configs:
        del built[:]
        with Patches(patches):
            keep = run(root)  # (the session must outlive describe())
        text = describe(built)
        n_launch = sum(len(p.fwd) + len(p.bwd) for p in built)
        print(f"{name} {hashlib.sha256(text.encode()).hexdigest()[:24]} plans={len(built)} launches={n_launch}", flush=True)
        if args.dump:
            with open(os.path.join(args.dump, name.replace("/", "_").replace(",", "+") + ".txt"), "w") as f:
                f.write(text)
        del built[:], keep
    print(f"{len(configs)} configurations", flush=True)


if __name__ == "__main__":
    main()
