"""-m gpu: the nine entry points of csrc/capsule.hip through the C-ABI against a float64 autograd reference that shares
no backward algebra with them (tests/capsule_cases.py; the same cases through the emulation twins in
tests/test_capsule_cases_emu.py).  k1 shapes: more than 256 prediction columns with every capsule count and batch size at
which a loop or a tile changes, strided views, canaries around every output; k2 squash edges, per capsule vector; k3
routing logits where only float64 holds; k4 refusals before any launch; k5 a training step through the planner above 256
columns.  Every case runs twice on identical inputs and must give the same bits."""
import numpy as np
import pytest

from hypelcnn_amd.backend import HypelError, Ref
from tests import capsule_cases as C
from tests import emu_capsule as EC
from tests import parity_util as PU

pytestmark = pytest.mark.gpu
TOL_LOGIT, TOL_GRAD = 1e-3, 5e-4  # tests/test_gpu_capsule.py

# The yardstick of the edge cases: the error of a plain float32 NumPy rendition of the kernels' closed forms
# (capsule_cases.F32R; float64 only where the contract says so) against the float64 reference, per capsule vector (per
# row of the [I, J] tensors) relative to that vector's largest reference entry, largest over the case.  A kernel is
# allowed C.MARGIN = 4 x that: it sums in another order, and that is all the margin pays for.  0 = the rendition is
# exact there, and so must the kernel be.  DESIGN.md 3.4 "Errors at the edges" holds the same rows next to what the
# kernels showed on an MI355X; tests/test_capsule_cases_emu.py re-measures the rendition against these constants.
# squash: one column per regime of capsule_cases.SQUASH_Q (q = 0, 1e-14, 1e-10, 1e-9, 1e-8, 1e-4, 1 - 1e-3, 1 + 1e-3, 1e2, 1e8).
# head_bwd with gy alone at q >= 1e2: dv is parallel to s, and gain * dv + gain' * (2/D) <s, dv> s cancels to 1/q of its
# terms (|v| saturates) -- the float32 closed form returns rounding noise of those terms there, in the rendition as in
# the kernel; the true gradient is 1e-12 of gy at q = 1e8.
EDGE_F32_ERR = {
    "squash": {
        "route_fwd.s": [0.0, 2.1e-07, 1.1e-07, 7.9e-08, 9.7e-08, 1.1e-07, 1.3e-07, 1.3e-07, 1.6e-07, 1.2e-07],
        "route_fwd.v": [0.0, 2.8e-07, 1.8e-07, 1.1e-07, 1.2e-07, 1.5e-07, 1.4e-07, 2.2e-07, 1.4e-07, 1.6e-07],
        "route_fwd.y": [0.0, 2.1e-07, 2.2e-07, 1.1e-07, 8.9e-08, 1.4e-07, 9.7e-08, 1.1e-07, 6.4e-08, 5.0e-08],
        "route_bwd": [0.0, 1.4e-07, 1.1e-07, 1.4e-07, 1.3e-07, 2.0e-07, 1.9e-07, 2.2e-07, 1.7e-07, 1.8e-07],
        "head_bwd": [0.0, 9.2e-08, 1.6e-07, 1.3e-07, 1.3e-07, 1.5e-07, 8.4e-08, 1.6e-07, 1.8e-07, 9.9e-08],
        "head_bwd_gy": [0.0, 7.5e-08, 1.2e-07, 1.5e-07, 1.7e-07, 2.0e-07, 1.2e-07, 3.0e-07, 7.1e-06, 6.4e+00],
        "head_bwd_gv": [0.0, 8.7e-08, 1.1e-07, 9.8e-08, 8.1e-08, 1.4e-07, 5.2e-08, 1.7e-07, 1.3e-07, 1.4e-07],
    },
    # logits: per row of the [I, J] tensor; b is a float64 buffer
    "logits": {
        "agree_fwd.b": 5.2e-16, "agree_fwd.c": 4.1e-08, "agree_fwd.b_nob": 5.2e-16, "agree_fwd.c_nob": 5.1e-08,
        "agree_bwd": 6.5e-08, "agree_bwd_nonext": 9.2e-08,
    },
}


def edge_f32(case, key):
    return EDGE_F32_ERR[case][key[0]][key[1]] if isinstance(key, tuple) else EDGE_F32_ERR[case][key]


def edge_limit(case, key):
    return C.MARGIN * edge_f32(case, key)


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


# ------------------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_k1_every_entry_point_at_wide_and_ragged_shapes(hip, shape):
    """capsule_cases.shape_case: each output within KERNEL_TOL of its largest float64 entry, nothing outside the
    contract's extent written (guards, pad columns of dx and of the mask operands), two runs bit-identical."""
    case = C.get(shape)
    res = case.run(hip)
    errs = case.errors(res)
    print("\n" + case.name + ": " + ", ".join(f"{k} {e:.1e}" for k, (e, _, _) in errs.items()))
    for label, (err, _, _) in errs.items():
        assert err < C.KERNEL_TOL, (label, err)
    C.assert_same_bits(res, case.run(hip))


# ------------------------------------------------------------------------------------------------- 2./3. edge regimes
@pytest.mark.parametrize("name", ["squash", "logits"])
def test_k2_k3_edge_regimes_per_vector(hip, name):
    """squash: whole capsules at q = 0 (s, v, y, ds exactly zero, with gy given too), 1e-14 .. 1e-8 around eps, 1 -+ 1e-3,
    up to 1e8.  logits: b of several hundred, gaps of 800 (coefficients exactly 0 and 1), equal logits, dc = 1e4 + O(1)
    with saturated, uniform and spread coefficients.  Limits: edge_limit()."""
    case = C.get(name)
    res = case.run(hip)
    errs = case.errors(res)  # asserts the canaries, finiteness and the exact zeros
    for label, (err, _, key) in errs.items():
        print(f"{name} {label}: device {err:.3e}, fp32 rendition {edge_f32(name, key):.3e}, limit {edge_limit(name, key):.3e}")
    for label, (err, _, key) in errs.items():
        assert err <= edge_limit(name, key), (label, err)
    C.assert_same_bits(res, case.run(hip))


# ---------------------------------------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("refusal", C.REFUSALS, ids=C.refusal_id)
def test_k4_refused_before_any_launch(hip, refusal):
    entry, _, change = refusal
    args, bufs, outs = C.refusal_args(entry, change)
    store = {k: hip.upload(v) for k, v in bufs.items()}
    with pytest.raises(HypelError, match="hypel_" + entry):
        hip.call(entry, *[Ref(store[a]) if isinstance(a, str) else a for a in args])
    hip.synchronize()
    for k in outs:
        if k in store:
            got = store[k].cpu().numpy()
            assert (got.view(np.uint8) == bufs[k].view(np.uint8)).all(), k


def test_k4_the_baseline_calls_of_the_refusal_table_run(hip):
    """... so that each refusal is owed to the one argument it changes"""
    for entry in C.BASELINE:
        args, bufs, outs = C.refusal_args(entry, {})
        store = {k: hip.upload(v) for k, v in bufs.items()}
        hip.call(entry, *[Ref(store[a]) if isinstance(a, str) else a for a in args])
        hip.synchronize()
        assert any((store[k].cpu().numpy().view(np.uint8) != bufs[k].view(np.uint8)).any() for k in outs), entry


# ------------------------------------------------------------------------------------------------------- 5. model level
@pytest.mark.parametrize("classes,width,seed", C.MODEL_CASES)
def test_k5_training_step_above_256_columns(hip, classes, width, seed):
    alg, params, x, onehot = C.model_inputs(classes, width, seed)
    built = PU.build("CAPModel", C.MODEL_PATCH, C.MODEL_CHANNELS, classes, alg, hip, with_eval=False)
    sess = built.ctx.session()
    PU.inject(sess, params)
    ct = PU.run_train_step(built, x, onehot, {})
    ref = EC.torch_capsule_step(params, x, onehot, classes, alg, True)
    assert ref["qmin"] > 1e-6 and min(float(p.abs().min()) for p in ref["pre"].values()) > EC.KINK_ZONE
    assert EC.product_relu_decisions(built, ct, ref["pre"]) == ({}, 0)
    err = np.abs(ct.value(built.y_conv).cpu().numpy() - ref["logits"]).max()
    errs = {k: np.abs(sess.get_gradient("nn_core/" + k) - g).max() / max(np.abs(g).max(), 1e-6) for k, g in ref["grads"].items()}
    worst = max(errs.items(), key=lambda t: t[1])
    print(f"\nCAPModel {classes} x {width}: logit err {err:.2e}, worst gradient {worst[0]} {worst[1]:.2e}")
    assert err < TOL_LOGIT
    assert abs(ct.loss_value() - ref["loss"]) < TOL_LOGIT * max(1.0, abs(ref["loss"]))
    assert worst[1] < TOL_GRAD, worst
