"""-m gpu: the capsule kernels (csrc/capsule.hip) one by one against their emulation twins (tests/emu_capsule.py) on
ragged sizes, and the whole CAPModel step against the reference fixture and a float64 torch restatement
(tests/emu_capsule.torch_capsule_step) at the project's limits: logits 1e-3 absolute, every gradient within 5e-4 of that
tensor's largest entry."""
import json
import os

import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import Ref
from oracle import train as OT
from tests import emu_capsule as EC
from tests import parity_util as PU
from tests.emu_backend import EmuBackend

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_LOGIT, TOL_GRAD = 1e-3, 5e-4
KERNEL_TOL = 2e-5  # one kernel, fp32 sums of at most a few thousand terms, relative to the output's largest entry
SHIPPED = json.load(open(os.path.join(GOLDEN, "alg_param_capn.json")))
GRSS2013 = dict(patch=7, channels=145, classes=15)
EVAL_SEED = 11  # every sample's top-two margin exceeds the logit limit at batch 16 (checked in float64 on the CPU)


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


class Pair:
    """The same named float buffers on the device and on the host; runs an entry point on both and compares outputs."""

    def __init__(self, hip, rng):
        self.hip, self.emu, self.rng = hip, EmuBackend(), rng
        self.dev, self.host = {}, {}

    def add(self, name, array):
        a = np.ascontiguousarray(array)
        self.host[name] = torch.from_numpy(a.reshape(-1).copy())
        self.dev[name] = self.host[name].to(self.hip.device)

    def rand(self, name, *shape, scale=1.0):
        self.add(name, (self.rng.standard_normal(shape) * scale).astype(np.float32))

    def zeros(self, name, n):
        self.add(name, np.zeros(n, np.float32))

    def run(self, entry, args, outputs):
        def resolve(store):
            return [None if a is None else (Ref(store[a[0]], a[1]) if isinstance(a, tuple) else
                                            Ref(store[a]) if isinstance(a, str) else a) for a in args]
        self.hip.call(entry, *resolve(self.dev))
        self.hip.synchronize()
        self.emu.call(entry, *resolve(self.host))
        for name in outputs:
            got, want = self.dev[name].cpu().numpy(), self.host[name].numpy()
            scale = max(np.abs(want).max(), 1e-6)
            err = np.abs(got - want).max() / scale
            assert err < KERNEL_TOL, (entry, name, err)
            self.dev[name].copy_(self.host[name])  # the next kernel starts from identical inputs


# N not a multiple of the 16-sample tile or the wave split, I not a multiple of the wave, J*D not a multiple of 64
@pytest.mark.parametrize("n,pixels,m,j,d,terms", [(19, 5, 3, 5, 6, 3), (70, 7, 5, 7, 16, 5), (1, 2, 1, 2, 3, 1),
                                                  (33, 9, 32, 15, 16, 5)])
def test_each_kernel_against_its_emulation_twin(hip, n, pixels, m, j, d, terms):
    rng = np.random.default_rng(n * 131 + j)
    i, jd, ld = pixels * m, j * d, m * d + 3
    p = Pair(hip, rng)
    # the primary capsules: a channel-offset view of a wider pixel-major buffer, pixels in a shuffled order
    pix = (rng.permutation(pixels).astype(np.int64) * n * ld + 2)
    p.add("pix", pix)
    p.rand("x", pixels * n * ld)
    p.rand("w", i, d, jd, scale=0.5)
    p.rand("bias", i, jd, scale=0.1)
    p.zeros("uhat", n * i * jd)
    p.run("caps_uhat_fwd", ["x", "pix", ld, m, "w", "bias", n, i, d, jd, "uhat"], ["uhat"])
    coef = rng.random((i, j)).astype(np.float32)
    p.add("coef", coef / coef.sum(1, keepdims=True))
    for name in ("s", "v", "ds"):
        p.zeros(name, n * jd)
    p.zeros("y", n * j)
    p.run("caps_route_fwd", ["uhat", "coef", n, i, j, d, "s", "v", "y"], ["s", "v", "y"])
    p.run("caps_route_fwd", ["uhat", "coef", n, i, j, d, "s", "v", None], ["s", "v"])
    p.add("b_in", rng.standard_normal((i, j)) * 0.3)  # the routing logits are fp64 buffers
    p.add("b_out", np.zeros(i * j, np.float64))
    p.zeros("c_out", i * j)
    p.run("caps_agree_fwd", ["uhat", "v", n, i, j, d, "b_in", "b_out", "c_out"], ["b_out", "c_out"])
    p.run("caps_agree_fwd", ["uhat", "v", n, i, j, d, None, "b_out", "c_out"], ["b_out", "c_out"])
    p.rand("gy", n, j)
    p.rand("gv", n, jd)
    p.run("caps_head_bwd", ["gy", "gv", "s", n, j, d, "ds"], ["ds"])
    p.run("caps_head_bwd", ["gy", None, "s", n, j, d, "ds"], ["ds"])
    p.rand("db_next", i, j, scale=0.2)
    p.zeros("db", i * j)
    p.run("caps_agree_bwd", ["uhat", "ds", n, i, j, d, "c_out", "db_next", "db"], ["db"])
    p.run("caps_agree_bwd", ["uhat", "ds", n, i, j, d, "c_out", None, "db"], ["db"])
    p.zeros("ds_prev", n * jd)
    p.run("caps_route_bwd", ["uhat", "db", n, i, j, d, "s", "ds_prev"], ["ds_prev"])
    p.rand("coefs", terms, i, j, scale=0.3)
    p.rand("vecs", terms, n, jd)
    p.rand("dw", i, d, jd)
    p.rand("dbias", i, jd)
    p.rand("dx", pixels * n * ld)
    for acc in (0, 1):
        p.run("caps_uhat_bwd", ["x", "pix", ld, m, "w", n, i, j, d, terms, "coefs", "vecs", "dw", "dbias", acc, "dx", "pix",
                                ld, acc], ["dw", "dbias", "dx"])
    p.run("caps_uhat_bwd", ["x", "pix", ld, m, "w", n, i, j, d, terms, "coefs", "vecs", "dw", "dbias", 0, None, None, 0, 0],
          ["dw", "dbias"])
    p.rand("labels", n, j)
    p.zeros("masked", n * (d + 1))
    p.run("caps_mask_fwd", ["v", jd, "labels", j, n, j, d, "masked", d + 1], ["masked"])
    p.rand("gmask", n, d)
    for acc in (0, 1):
        p.run("caps_mask_bwd", ["gmask", d, "labels", j, n, j, d, "gv", jd, acc], ["gv"])


def _fixture():
    with open(os.path.join(GOLDEN, "reference_capsule.json")) as f:
        return json.load(f), np.load(os.path.join(GOLDEN, "reference_capsule.npz"))


@pytest.mark.parametrize("case", ["k1_decoder_r3", "k3_plain_r2", "k1_k3_plain_r1"])
def test_training_step_equals_the_reference_fixture(hip, case):
    meta, arrays = _fixture()
    c = meta["cases"][case]
    built = PU.build("CAPModel", c["patch"], c["channels"], c["classes"], c["algorithm_params"], hip)
    params, x, onehot, grads = EC.load_fixture_case(meta, arrays, case)
    sess = built.ctx.session()
    for k, v in params.items():
        sess.set_variable(k, v)
    ct = PU.run_train_step(built, x, onehot, {})
    err = np.abs(ct.value(built.y_conv).cpu().numpy() - arrays[f"{case}/y_conv"]).max()
    worst = 0.0
    for name, (want, index) in grads.items():
        got = sess.get_gradient(name).reshape(-1)
        got = got[index] if index is not None else got
        worst = max(worst, np.abs(got - want.reshape(-1)).max() / max(np.abs(want).max(), 1e-6))
    print(f"\n{case}: logit err {err:.2e}, loss {ct.loss_value():.6f} vs {c['loss']:.6f}, worst gradient {worst:.2e}")
    assert err < TOL_LOGIT
    assert abs(ct.loss_value() - c["loss"]) < TOL_LOGIT * max(1.0, abs(c["loss"]))
    assert worst < TOL_GRAD


def test_evaluation_tower_equals_the_reference_fixture(hip):
    meta, arrays = _fixture()
    c = meta["cases"]["evaluation_r3"]
    built = PU.build("CAPModel", c["patch"], c["channels"], c["classes"], c["algorithm_params"], hip)
    params, x, _, _ = EC.load_fixture_case(meta, arrays, "evaluation_r3")
    sess = built.ctx.session()
    for k, v in params.items():
        sess.set_variable(k, v)
    before = sess.state.clone()
    y = PU.run_eval(built, x)
    assert np.abs(y - arrays["evaluation_r3/y_conv"]).max() < TOL_LOGIT
    assert torch.equal(sess.state, before)


def _shipped(hip, nb, seed, **over):
    alg = dict(SHIPPED, **over)
    g = GRSS2013
    rng = np.random.default_rng(seed)
    built = PU.build("CAPModel", g["patch"], g["channels"], g["classes"], alg, hip)
    params = EC.init_params(g["patch"], g["channels"], g["classes"], alg, rng, alg["enable_decoding"])
    sess = built.ctx.session()
    PU.inject(sess, params)
    x = rng.random((nb, g["patch"], g["patch"], g["channels"])).astype(np.float32)
    onehot = np.eye(g["classes"], dtype=np.float32)[rng.integers(0, g["classes"], nb)]
    return built, sess, params, x, onehot, alg


@pytest.mark.parametrize("nb", [16, 128])
def test_shipped_configuration_step_against_float64(hip, nb):
    """Observed on an MI355X: batch 16 -- logits 7.8e-7, worst gradient 2.0e-5; batch 128 -- logits 8.2e-7 and, before
    pinning, `PrimaryCaps_layer/weights` at 5.4e-4 of its maximum, above the 5e-4 limit.  Cause: ONE of the 4.8 million
    ReLU pre-activations lies within fp32 rounding of zero and takes the other branch than float64, which moves a
    batch-normalised filter gradient by a discrete amount (a float64 run whose input is perturbed by 7e-7 shows the same
    5.5e-4 from one flip, and 1.1e-4 once it is pinned).  As for the leaky-ReLU models (parity_util.compare_step), the
    product's own branch decisions are read back, must differ from float64 only where |pre-activation| < 1e-4, and are
    pinned in the restatement; then every gradient must be inside the limit."""
    built, sess, params, x, onehot, alg = _shipped(hip, nb, 7)
    ct = PU.run_train_step(built, x, onehot, {})
    logits = ct.value(built.y_conv).cpu().numpy()
    grads = {k: sess.get_gradient("nn_core/" + k) for k in params if not k.endswith(("moving_mean", "moving_variance"))}
    ref = EC.torch_capsule_step(params, x, onehot, GRSS2013["classes"], alg, True)
    assert ref["qmin"] > 1e-6

    def worst_of(r):
        errs = {k: np.abs(grads[k] - g).max() / max(np.abs(g).max(), 1e-6) for k, g in r["grads"].items()}
        return max(errs.items(), key=lambda t: t[1])

    unpinned = worst_of(ref)
    force_all, history = {}, []
    for _ in range(4):  # pinning a decision moves everything behind it by a rounding-sized amount: repeat until stable
        force, flips = EC.product_relu_decisions(built, ct, ref["pre"])
        new = {k: v for k, v in force.items() if k not in force_all or not torch.equal(force_all[k], v)}
        history.append(flips)
        if not new:
            break
        force_all.update(new)
        ref = EC.torch_capsule_step(params, x, onehot, GRSS2013["classes"], alg, True, kink_force=force_all)
    err = np.abs(logits - ref["logits"]).max()
    worst = worst_of(ref)
    print(f"\nCAPModel GRSS2013 batch {nb}: logit err {err:.2e}, loss {ct.loss_value():.6f} vs {ref['loss']:.6f}, "
          f"worst gradient {worst[0]} {worst[1]:.2e} (unpinned {unpinned[1]:.2e}, ReLU flips per pass {history})")
    assert err < TOL_LOGIT
    assert abs(ct.loss_value() - ref["loss"]) < TOL_LOGIT * max(1.0, abs(ref["loss"]))
    assert worst[1] < TOL_GRAD, worst
    # two runs of the same step give identical bits
    ct = PU.run_train_step(built, x, onehot, {})
    assert np.array_equal(ct.value(built.y_conv).cpu().numpy(), logits)
    for k, g in grads.items():
        assert np.array_equal(sess.get_gradient("nn_core/" + k), g), k


def test_three_adam_steps_follow_the_float64_restatement(hip):
    """TF1 Adam moves a weight by about lr * sign(g) in its first steps, so a gradient within rounding of zero may move
    its weight the other way: after three steps every element lies within 3 * 2.01 lr of the float64 trainer's, and more
    than 99 % of them within 1 % of lr (the criterion of the HYPELCNN model-level Adam test)."""
    over = dict(feature_count=32, primary_capsule_count=4)
    built, sess, params, x, onehot, alg = _shipped(hip, 16, 3, **over)
    lr = alg["learning_rate"]
    p64 = {k: v.copy() for k, v in params.items()}
    names = [k for k in p64 if not k.endswith(("moving_mean", "moving_variance"))]
    m = {k: np.zeros_like(p64[k]) for k in names}
    v = {k: np.zeros_like(p64[k]) for k in names}
    for step in range(3):
        PU.run_train_step(built, x, onehot, {})
        sess.adam_step(built.lr.eval(sess.global_step))
        ref = EC.torch_capsule_step(p64, x, onehot, GRSS2013["classes"], alg, True)
        for k in names:
            OT.adam_tf1_step(p64[k], ref["grads"][k], m[k], v[k], lr, step + 1)
    n_close = n_all = 0
    for k in names:
        got = sess.get_variable("nn_core/" + k)
        slack = 2e-7 * max(1.0, np.abs(p64[k]).max())
        assert np.abs(got - p64[k]).max() <= 3 * 2.01 * lr + slack, k
        n_close += int((np.abs(got - p64[k]) <= 1e-2 * lr + slack).sum())
        n_all += got.size
    print(f"\n3 Adam steps: {n_all - n_close} of {n_all} elements differ by more than 1 % of lr")
    assert n_close / n_all > 0.99 and sess.global_step == 3


def test_evaluation_logits_and_labels_at_the_shipped_configuration(hip):
    built, sess, _, _, _, alg = _shipped(hip, 16, EVAL_SEED)
    g = GRSS2013
    rng = np.random.default_rng(EVAL_SEED)
    params = EC.init_params(g["patch"], g["channels"], g["classes"], alg, rng, True)
    x = rng.random((16, g["patch"], g["patch"], g["channels"])).astype(np.float32)
    # a class-dependent offset shared by every capsule's bias: with purely random maps the 1 568 predictions average out
    # and all classes tie within the logit limit
    offset = (rng.standard_normal(g["classes"] * alg["digit_capsule_output_space"]) * 0.3).astype(np.float32)
    for k in params:
        if "DigitCaps_layer_w_" in k and k.endswith("biases"):
            params[k] = (params[k] + offset).astype(np.float32).astype(np.float64)
    PU.inject(sess, params)
    want = EC.torch_capsule_eval(params, x, GRSS2013["classes"], alg)
    top = np.sort(want, 1)
    assert (top[:, -1] - top[:, -2]).min() > TOL_LOGIT, "pick another EVAL_SEED: a top-two margin is inside the logit limit"
    before = sess.state.clone()
    got = PU.run_eval(built, x)
    assert np.abs(got - want).max() < TOL_LOGIT
    assert (got.argmax(1) == want.argmax(1)).all()
    assert torch.equal(sess.state, before)
