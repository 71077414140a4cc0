"""The GAN wrappers' wiring, pinned by EXECUTING the reference's gan/wrappers/*.py (round-5 verdict: until now it reached
oracle/gan.py and hypelcnn_amd/gan/wrappers/* by reading only).

`tests/golden/make_reference_gan_wiring.py` ran the reference's unchanged wrapper files, `wrapper_registry.get_wrapper_dict`
and `shadow_data_models.py` under a recording `tensorflow_gan` / `tf` stand-in (`tests/golden/tfgan_standin.py`:
tensorflow_gan's functions restated after its published source) and committed what came out as data:
per train op the loss as weighted primitive terms with operands by provenance, the trained variables, Adam's beta1, the LR
schedule, tensor-pool use, float64 losses and gradients.  Held to it here:

  * `oracle/gan.py` -- phase order, trained variables, loss values and gradients of every phase (1e-10);
  * `oracle/host.py::gan_lr` and the product's `_get_lr` -- the LR schedule at the sampled steps;
  * the product's wrappers (`hypelcnn_amd.gan.wrapper_registry`) -- phase order, the terms of every phase with operands by
    provenance (walked back through the product's recorded graph), weights / targets / tau, the regularised variables, the
    trained variable groups, which LR each phase runs at, which phases feed the tensor pool;
  * the product's numbers on the kernel emulation against the reference-executed float64 values (5e-5).

`tests/golden/make_reference_facade.py` also recorded the phases the reference's wrapper files define through the
product's tensorflow_gan facade (reference_facade.json); the product's wrappers are held to those as well."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import gan as OG
from oracle.host import gan_lr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
FIX = json.load(open(os.path.join(GOLD, "reference_gan_wiring.json")))
ARR = np.load(os.path.join(GOLD, "reference_gan_wiring.npz"))
CASES = sorted(FIX)
FACADE = json.load(open(os.path.join(GOLD, "reference_facade.json")))["gan_phases"]
sys.path.insert(0, GOLD)


def _arrays(case, prefix):
    pre = f"{case}/{prefix}"
    return {k[len(pre):]: ARR[k] for k in ARR.files if k.startswith(pre)}


def _cfg(case):
    c = FIX[case]
    f = c["flags"]
    return OG.GanConfig(c["gan_type"], c["bands"], cycle_weight=f["cycle_consistency_loss_weight"],
                        identity_weight=f["identity_loss_weight"], use_identity=f["use_identity_loss"],
                        nce_weight=f["nce_loss_weight"], tau=f["tau"], patches=f["patches"], embed=f["embedded_feat_size"],
                        dis_reg=f["discriminator_reg_scale"], feat_reg=f["gen_disc_reg_scale"], generator_lr=f["generator_lr"],
                        discriminator_lr=f["discriminator_lr"], gen_discriminator_lr=f["gen_discriminator_lr"],
                        max_steps=c["max_steps"])


def _term_key(t):
    if t["kind"] == "l2":
        return ("l2", t["variable"], round(t["scale"], 12))
    ab = (t["a"], t.get("b"))
    if t["kind"] == "mean_abs":
        ab = tuple(sorted(ab))
    return (t["kind"],) + ab + (t.get("target"), t.get("tau"))


def _hook_terms(hook):
    """The distinct terms of a hook's train ops with their weights (two ops of one hook share the auxiliary terms)."""
    out = {}
    for op in hook["ops"]:
        for t in op["terms"]:
            k = _term_key(t)
            assert out.setdefault(k, t)["weight"] == t["weight"], k
    return out


# ------------------------------------------------------------------------------------------------ oracle/gan.py
@pytest.mark.parametrize("case", CASES)
def test_oracle_phases_equal_the_executed_reference_wrappers(case):
    c = FIX[case]
    cfg = _cfg(case)
    params = _arrays(case, "param/")
    x, y = ARR[f"{case}/x"], ARR[f"{case}/y"]
    phases = OG.phase_list(cfg.kind)
    assert len(phases) == len(c["hooks"]), (phases, len(c["hooks"]))
    names = OG.gan_param_names(cfg.kind, cfg.bands, cfg.patches, cfg.embed)
    assert sorted(params) == sorted(n for g in names.values() for vs in g.values() for n in vs) == sorted(c["variables"])
    for hi, (phase, hook) in enumerate(zip(phases, c["hooks"])):
        assert hook["train_steps"] == 1
        loss, grads = OG.phase_gradients(cfg, params, x, y, phase)
        trained = [v for op in hook["ops"] for v in op["variables"]]
        assert sorted(grads) == sorted(trained), (phase, sorted(set(grads) ^ set(trained)))
        want_loss = sum(t["weight"] * t["value"] for t in _hook_terms(hook).values())
        if len(hook["ops"]) == 1:
            assert abs(want_loss - hook["ops"][0]["loss"]) <= 1e-12 * max(1.0, abs(want_loss))
        assert abs(loss - want_loss) <= 1e-10 * max(1.0, abs(want_loss)), (case, phase, loss, want_loss)
        for oi, op in enumerate(hook["ops"]):
            for vn in op["variables"]:
                want = ARR[f"{case}/hook{hi}/op{oi}/grad/{vn}"]
                scale = max(1e-12, float(np.abs(want).max()))
                assert np.abs(grads[vn] - want).max() <= 1e-9 * max(scale, 1e-6), (case, phase, vn)
    # the reference's own execution shows the discarded coupling of the DCL wrappers (dcl_gan_wrapper.py:189-190,
    # dcl_cycle_gan_wrapper.py:149-150): no term of one direction's generator loss mentions the other direction's networks
    if cfg.kind in ("dcl_gan", "dcl_cycle_gan"):
        for hook, tag in ((c["hooks"][0], "ModelY2X"), (c["hooks"][3], "ModelX2Y")):
            assert not any(tag in json.dumps(t) for t in hook["ops"][0]["terms"])
            assert not any(t["kind"] == "mean_abs" for t in hook["ops"][0]["terms"])  # ... and no cycle term was added


@pytest.mark.parametrize("case", CASES)
def test_lr_schedule_and_optimiser_settings(case):
    from hypelcnn_amd.gan.wrappers.gan_common import _get_lr
    c = FIX[case]
    f = c["flags"]
    base_of = {"Generator": f["generator_lr"], "Discriminator": f["discriminator_lr"], "FeatDiscriminator": f["gen_discriminator_lr"]}
    for hook in c["hooks"]:
        for op in hook["ops"]:
            group = op["variables"][0].split("/")[-3]
            assert all(v.split("/")[-3] == group for v in op["variables"])
            base = base_of[group]
            assert (op["beta1"], op["beta2"], op["epsilon"]) == (0.5, 0.999, 1e-8)
            product = _get_lr(base, c["max_steps"])
            for s, want in zip(c["lr_steps"], op["lr"]):
                assert abs(gan_lr(base, s, c["max_steps"]) - want) <= 1e-18, (s, want)
                assert abs(product(s) - want) <= 1e-18, (s, want)


# ------------------------------------------------------------------------------------------------ the product's wrappers
def _build_product(case, backend):
    from hypelcnn_amd.gan.wrapper_registry import get_wrapper_dict
    from hypelcnn_amd.gan.wrappers import gan_common as C
    c = FIX[case]
    f = c["flags"]
    wrapper = get_wrapper_dict(SimpleNamespace(**f))[c["gan_type"]]
    wrapper.backend = backend
    tower, x, y = C.new_gan_tower(c["bands"])
    model = wrapper.define_model(x, y)
    loss = wrapper.define_loss(model)
    ops = wrapper.define_train_ops(model, loss, max_number_of_steps=c["max_steps"], generator_lr=f["generator_lr"],
                                   discriminator_lr=f["discriminator_lr"], gen_discriminator_lr=f["gen_discriminator_lr"])
    ops.capture_graphs = False
    return wrapper, model, loss, ops


def _label(t, pool_of):
    """Provenance of a tensor of the product's recorded graph, in the fixture's notation."""
    from hypelcnn_amd import graph as G
    if t.root is not None and t.node is None:
        return _label(t.root, pool_of)
    n = t.node
    if n is None:
        return f"pool({pool_of[t.name]})" if t.name in pool_of else t.name
    if isinstance(n, G.GeneratorNode):
        scope = n.weights[0].name.rsplit("/", 2)[0]
        return f"{'E' if n.only_encoder else 'G'}[{scope}]({_label(n.src, pool_of)})"
    # discriminator / feature discriminator: walk down the dense layers to the network's input
    var, cur = None, t
    while True:
        n = cur.node
        if isinstance(n, G.DenseStackNode):
            var, cur = n.layers[0][0], n.src
        elif isinstance(n, G.FeatStackNode):
            cur = n.srcs[0]
        elif isinstance(n, G.LinearNode):
            var, cur = n.branches[0].w, n.sources[0]
        elif n is None and cur.root is not None:
            cur = cur.root
        else:
            break
        if cur.node is None and cur.root is None or isinstance(cur.node, G.GeneratorNode):
            break
        if cur.root is not None and cur.node is None and (cur.root.node is None or isinstance(cur.root.node, G.GeneratorNode)):
            cur = cur.root
            break
    scope = G.group_of(var.name)
    kind = {"Discriminator": "D", "FeatDiscriminator": "F"}[scope.rsplit("/", 1)[-1]]
    return f"{kind}[{scope}]({_label(cur, pool_of)})"


@pytest.mark.parametrize("case", CASES)
def test_product_phases_equal_the_executed_reference_wrappers(case):
    from tests.emu_backend import EmuBackend
    c = FIX[case]
    wrapper, model, loss, ops = _build_product(case, EmuBackend())
    sess = ops.ctx.session()
    assert sorted(sess.variable_names()) == sorted(c["variables"])
    by_name = {v.name: v for v in loss.tower.store.order}
    assert {n: list(by_name[n].shape) for n in c["variables"]} == c["variables"]
    assert sorted((n, round(v.l2_scale, 12)) for n, v in by_name.items() if v.l2_scale) == \
        sorted((n, round(s, 12)) for n, s in c["regularised"])
    assert len(loss.phases) == len(c["hooks"])
    for phase, hook in zip(loss.phases, c["hooks"]):
        pool_of = {name: _label(t, {}) for name, t in (phase.pool or [])}
        # (a term the reference multiplies by 0.0 -- the identity NCE with use_identity_loss off, cut_wrapper.py:593 -- is
        # not built by the product: same loss, same gradients, three network applications less)
        want = {k: t for k, t in _hook_terms(hook).items() if t["weight"] != 0.0}
        got = {}
        for t in phase.terms:
            d = {"kind": t.kind, "a": _label(t.a, pool_of), "b": None if t.b is None else _label(t.b, pool_of),
                 "target": t.target if t.kind == "mean_sq" else None, "tau": t.tau if t.kind == "nce" else None}
            k = _term_key(d)
            assert k not in got, k
            got[k] = t.weight
        trained = sorted(v for op in hook["ops"] for v in op["variables"])
        groups = [g if isinstance(g, str) else g.name for g in phase.train_groups]
        mine = sorted(n for n in by_name if any(n.startswith(g + "/") for g in groups))
        assert mine == trained, (phase.name, groups)
        for n in mine:  # tfgan.gan_loss / cut_loss add the trained scope's regularisation losses
            if by_name[n].l2_scale:
                got[("l2", n, round(by_name[n].l2_scale, 12))] = 1.0
        assert set(got) == set(want), (case, phase.name, sorted(set(got) ^ set(want), key=str))
        for k, w in got.items():
            assert abs(w - want[k]["weight"]) <= 1e-12, (k, w, want[k]["weight"])
        # which LR the phase runs at, and whether it feeds the tensor pool
        lr = ops.lrs[phase.lr_key]
        for s, v in zip(c["lr_steps"], hook["ops"][0]["lr"]):
            assert abs(lr(s) - v) <= 1e-18
        assert bool(phase.pool) == any("pool(" in json.dumps(t) for op in hook["ops"] for t in op["terms"])
        assert ops.use_pool == bool(c["pooled"]) or not phase.pool


@pytest.mark.parametrize("case", CASES)
def test_product_numbers_on_the_emulation_equal_the_executed_reference(case):
    """Loss value and every trained variable's gradient of every phase, at the fixture's parameters and inputs (rounded to
    fp32, as the device holds them): the product through planner + kernel emulation against the float64 values the
    REFERENCE's wrapper text produced.  (The float64 reference values are recomputed by the oracle at the fp32-rounded
    parameters; the previous test ties that oracle to the fixture at 1e-10.)"""
    from tests.emu_backend import EmuBackend
    from tests import gan_util as U
    c = FIX[case]
    cfg = _cfg(case)
    params = U.fp32(_arrays(case, "param/"))
    x = ARR[f"{case}/x"].astype(np.float32).astype(np.float64)
    y = ARR[f"{case}/y"].astype(np.float32).astype(np.float64)
    wrapper, model, loss, ops = _build_product(case, EmuBackend())
    assert [p.name for p in loss.phases] == OG.phase_list(cfg.kind)
    sess = ops.ctx.session()
    U.inject(sess, params)
    worst = U.check_phase_gradients(cfg, ops, params, x, y, tol=5e-5)
    assert worst < 5e-5


# ------------------------------------------------------------------------------------------------ the facade, end to end
def _canonical_phases(loss, ops, c):
    out = []
    by_name = {v.name: v for v in loss.tower.store.order}
    for phase in loss.phases:
        pool_of = {name: _label(t, {}) for name, t in (phase.pool or [])}
        terms = {}
        for t in phase.terms:
            d = {"kind": t.kind, "a": _label(t.a, pool_of), "b": None if t.b is None else _label(t.b, pool_of),
                 "target": t.target if t.kind == "mean_sq" else None, "tau": t.tau if t.kind == "nce" else None}
            terms[_term_key(d)] = round(t.weight, 12)
        groups = sorted(g if isinstance(g, str) else g.name for g in phase.train_groups)
        out.append({"name": phase.name, "terms": terms, "groups": groups, "lr": [ops.lrs[phase.lr_key](s) for s in c["lr_steps"]],
                    "pool": sorted(pool_of.items())})
    return out, sorted((n, list(v.shape), round(v.l2_scale, 12)) for n, v in by_name.items())


@pytest.mark.parametrize("case", CASES)
def test_reference_wrapper_files_build_the_products_phases(case):
    """`hypelcnn_amd.tfgan_facade.reference_wrapper`: the reference's UNCHANGED gan/wrapper_registry.py + gan/wrappers/*.py in
    the place of the product's wrapper -- define_model -> define_loss -> define_train_ops through the tensorflow_gan facade
    onto the product's graph -- as recorded by tests/golden/make_reference_facade.py: the product wrapper gives the same
    phases (names, terms with operands by provenance, weights, trained groups, LR schedule, tensor-pool feeds, variables
    with shapes and regulariser scales), and with them the oracle's numbers on the kernel emulation."""
    import make_reference_facade as MF
    from tests import gan_util as U
    from tests.emu_backend import EmuBackend
    c = FIX[case]
    _, _, loss_p, ops_p = _build_product(case, EmuBackend())
    got = MF.gan_phases_jsonable(_canonical_phases(loss_p, ops_p, c), bool(ops_p.use_pool))
    want = FACADE[case]
    assert got["variables"] == want["variables"]
    assert got["phases"] == want["phases"], (case, [(g["name"], w["name"]) for g, w in zip(got["phases"], want["phases"]) if g != w])
    assert got["use_pool"] == want["use_pool"]
    # ... and the numbers: every phase's loss and gradients against the oracle, through planner + kernel emulation
    cfg = _cfg(case)
    params = U.fp32(_arrays(case, "param/"))
    xv = ARR[f"{case}/x"].astype(np.float32).astype(np.float64)
    yv = ARR[f"{case}/y"].astype(np.float32).astype(np.float64)
    sess = ops_p.ctx.session()
    U.inject(sess, params)
    assert U.check_phase_gradients(cfg, ops_p, params, xv, yv, tol=5e-5) < 5e-5
