"""`optimize_nn` and the classifiers' `get_loss_func`, pinned by EXECUTING the reference's text.

`tests/golden/make_reference_optimize.py` ran `common/common_nn_ops.py:208-240` and the three plugin files' `get_loss_func`
unchanged under the float64 recording engine and committed: the optimiser's class / name / hyper-parameters, the LR at ten
steps, the loss value and every gradient of the train op's loss.  Held to it: `oracle/train.py::forward_backward` (loss and
gradients at 1e-10, the set of trained variables), `oracle/host.py::exponential_decay_staircase` and the product's
`LearningRate`, the product's optimiser settings, and the product's numbers on the kernel emulation."""
import json
import os

import numpy as np
import pytest

from oracle import train as OT
from oracle.host import exponential_decay_staircase

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
FIX = json.load(open(os.path.join(GOLD, "reference_optimize.json")))
ARR = np.load(os.path.join(GOLD, "reference_optimize.npz"))
CASES = sorted(FIX)
FACADE = json.load(open(os.path.join(GOLD, "reference_facade.json")))
FACADE_ARR = np.load(os.path.join(GOLD, "reference_facade.npz"))


def _arrays(case, prefix):
    pre = f"{case}/{prefix}"
    return {k[len(pre):]: ARR[k] for k in ARR.files if k.startswith(pre)}


@pytest.mark.parametrize("case", CASES)
def test_oracle_step_equals_the_executed_reference(case):
    c = FIX[case]
    params, masks = _arrays(case, "param/"), _arrays(case, "mask/")
    r = OT.forward_backward(c["model"], {k: v.copy() for k, v in params.items()}, ARR[f"{case}/x"], ARR[f"{case}/labels"],
                            c["classes"], c["alg"], True, masks)
    assert abs(r["loss"] - c["loss"]) <= 1e-11 * max(1.0, abs(c["loss"])), (r["loss"], c["loss"])
    np.testing.assert_allclose(r["logits"], ARR[f"{case}/logits"], rtol=1e-11, atol=1e-12)
    assert sorted(r["grads"]) == c["trained"] == sorted(OT.trainable_names(params))
    for k in c["trained"]:
        want = ARR[f"{case}/grad/{k}"]
        assert np.abs(r["grads"][k] - want).max() <= 1e-10 * max(1e-6, float(np.abs(want).max())), k
    # what the reference's loss text is made of: per-sample cross entropy (+ the scalar reconstruction MSE), then the mean
    tail = c["loss_ops"]
    assert tail[-1] == "reduce_mean" and "softmax_cross_entropy_with_logits" in tail
    assert (tail[-6:] == ["reshape", "sub", "square", "reduce_mean", "add", "reduce_mean"]) == (c["model"] == "HYPELCNNModel")
    assert c["create_train_op_kwargs"] == ["global_step"] or c["create_train_op_kwargs"] == []
    assert c["global_step_is_the_shared_one"]


@pytest.mark.parametrize("case", CASES)
def test_lr_schedule_and_optimiser(case):
    from hypelcnn_amd.common.common_nn_ops import LearningRate
    import inspect
    from hypelcnn_amd.runtime import Session
    c = FIX[case]
    alg = c["alg"]
    lr = LearningRate(alg["learning_rate"], alg["learning_rate_decay_step"], alg["learning_rate_decay_factor"])
    for s, want in zip(c["lr_steps"], c["lr"]):
        assert abs(exponential_decay_staircase(alg["learning_rate"], s, alg["learning_rate_decay_step"],
                                               alg["learning_rate_decay_factor"]) - want) <= 1e-15 * max(1.0, want)
        assert abs(lr.eval(s) - want) <= 1e-15 * max(1.0, want)
    opt = c["optimizer"]
    if isinstance(alg["optimizer"], (list, tuple)):
        assert opt["class"] == "MomentumOptimizer" and opt["name"] == "nn_core/Momentum"
        assert opt["hyper"] == {"momentum": alg["optimizer"][1], "use_nesterov": False}
    else:
        assert opt["class"] == "AdamOptimizer" and opt["name"] == "nn_core/Adam"
        d = inspect.signature(Session.adam_step).parameters
        assert opt["hyper"] == {"beta1": d["beta1"].default, "beta2": d["beta2"].default, "epsilon": d["eps"].default}


@pytest.mark.parametrize("case", CASES)
def test_product_step_on_the_emulation_equals_the_executed_reference(case):
    from tests import parity_util as U
    from tests.emu_backend import EmuBackend
    c = FIX[case]
    params = {k: v.astype(np.float32).astype(np.float64) for k, v in _arrays(case, "param/").items()}
    masks = _arrays(case, "mask/")
    x = ARR[f"{case}/x"].astype(np.float32)
    onehot = ARR[f"{case}/labels"].astype(np.float32)
    built = U.build(c["model"], c["patch"], c["channels"], c["classes"], c["alg"], EmuBackend())
    sess = built.ctx.session()
    U.inject(sess, params)
    ct = U.run_train_step(built, x, onehot, masks)
    # the float64 reference values at the fp32-rounded parameters come from the oracle, which the first test ties to the fixture
    U.compare_step(built, ct, params, x, onehot, masks, c["model"], c["classes"], c["alg"], tol_logit=2e-5, tol_grad=2e-4)
    assert sorted(k for k in c["trained"]) == sorted(v.name[len("nn_core/"):] for v in sess.trainable)


def test_shadow_ratio_augmentation_of_the_gan_input_equals_the_executed_reference():
    """`gan/gan_train_for_shadow.py:171-182` (perform_shadow_augmentation_random: with probability reg_support_rate the
    normal spectrum becomes shadow x ratio, then -- from the POSSIBLY REPLACED normal -- the shadow spectrum becomes
    normal / ratio) executed with its two uniform draws pinned (tests/golden/make_reference_facade.py recorded its
    outputs), against the product's pair kernel specification (`hypel_gather_pairs_f32`, tests/emu_backend.py) for all
    four branch combinations and a draw just below the rate."""
    import torch
    from hypelcnn_amd.backend import Ref
    from tests.emu_backend import EmuBackend
    a = {k[len("shadow_aug/"):]: FACADE_ARR[k] for k in FACADE_ARR.files if k.startswith("shadow_aug/")}
    rate = FACADE["shadow_augmentation"]["rate"]
    normal, shadow, ratio = a["normal"], a["shadow"], a["ratio"]
    bands = normal.size
    emu = EmuBackend()
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))  # noqa: E731
    for (u1, u2), x_ref, y_ref in zip(a["draws"], a["x"], a["y"]):
        ox, oy = torch.zeros(bands), torch.zeros(bands)
        emu.k_gather_pairs_f32(Ref(t(normal)), Ref(t(shadow)), Ref(torch.zeros(1, dtype=torch.int64)), 1, bands, Ref(t(ratio)),
                               Ref(t(np.float32([u1]))), Ref(t(np.float32([u2]))), rate, Ref(ox), Ref(oy))
        assert np.array_equal(ox.numpy(), x_ref) and np.array_equal(oy.numpy(), y_ref), (u1, u2)
    # the five draw pairs reach all four branches: each output is once the input and once the ratio-scaled spectrum
    assert {bool(np.array_equal(x, normal)) for x in a["x"]} == {True, False}
    assert {bool(np.array_equal(y, shadow)) for y in a["y"]} == {True, False}


def test_generator_as_augmenter_equals_the_executed_reference():
    """`gan/gan_utilities.py:30-43` (create_gan_struct) + `gan/wrappers/gan_common.py:282-304`
    (create_inference_for_matrix_input) + the reference's CycleGANInferenceWrapper and generator, executed in float64 on a
    [P, P, B + 1] patch by tests/golden/make_reference_facade.py -- P * P generator copies under
    Model/ModelX2Y|ModelY2X/Generator, the LiDAR channel passed through -- against the product's GeneratorAugmenter (ONE
    fused launch over all pixel spectra) on the kernel emulation, with the variables the reference's run created, for the
    shadowing and the de-shadowing direction."""
    import torch
    from hypelcnn_amd.gan.gan_utilities import GeneratorAugmenter
    from hypelcnn_amd.gan.wrapper_registry import get_infer_wrapper_dict
    from tests.emu_backend import EmuBackend
    rec = FACADE["generator_augmenter"]
    P, B = rec["P"], rec["B"]
    assert sorted({n.rsplit("/", 2)[0] for n in rec["variables"]}) == ["Model/ModelX2Y/Generator", "Model/ModelY2X/Generator"]
    assert len(rec["variables"]) == 28   # 2 x 7 layers x (weights, biases): P * P applications SHARE them
    pre = "gen_aug/param/"
    params = {k[len(pre):]: FACADE_ARR[k] for k in FACADE_ARR.files if k.startswith(pre)}
    assert sorted(params) == rec["variables"]
    patch = FACADE_ARR["gen_aug/patch"]
    outs = {True: FACADE_ARR["gen_aug/shadow"], False: FACADE_ARR["gen_aug/deshadow"]}
    for is_shadow in (True, False):
        aug = GeneratorAugmenter(get_infer_wrapper_dict()["cycle_gan"], is_shadow, B, EmuBackend())
        aug.load({k: np.asarray(v, np.float32) for k, v in params.items()})
        got = aug(torch.as_tensor(patch[None].astype(np.float32))).numpy()[0]
        want = outs[is_shadow]
        assert got.shape == want.shape == (P, P, B + 1)
        assert np.array_equal(got[..., -1], patch[..., -1].astype(np.float32)), "LiDAR channel must pass through"
        assert np.abs(got - want).max() < 2e-5 * max(1.0, np.abs(want).max()), (is_shadow, np.abs(got - want).max())
    assert np.abs(outs[True] - outs[False]).max() > 1e-3   # two different generators
