"""CPU: every case of tests/capsule_cases.py through the emulation twins (tests/emu_capsule.py) against the float64
autograd reference of the same file -- which ties the twins to something that does not share their backward algebra, and
is where the cases, their canaries and their limits are exercised without a GPU.  Then: the fp32 rendition's errors are
re-measured and held to the constants the GPU test derives its limits from; the logit cases defeat the float32
simplifications they are there for; the measures refuse a planted defect; the model-level cases sit where their seeds
were picked for (qmin, ReLU kinks)."""
import numpy as np
import pytest

from hypelcnn_amd import graph as G
from tests import capsule_cases as C
from tests import emu_capsule as EC
from tests import parity_util as PU
from tests.emu_backend import EmuBackend
from tests.test_gpu_capsule_kernels import EDGE_F32_ERR, TOL_GRAD, TOL_LOGIT, edge_f32, edge_limit


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_shape_cases_on_the_emulation(shape):
    case = C.get(shape)
    res = case.run(EmuBackend())
    for label, (err, _, _) in case.errors(res).items():
        assert err < C.KERNEL_TOL, (label, err)
    C.assert_same_bits(res, case.run(EmuBackend()))


def test_shape_table_covers_what_it_claims():
    wide = [s for s in C.SHAPES if s[3] * s[4] > 256]
    assert {s[1] * s[2] for s in wide} >= {1, 7, 8, 9, 31, 32, 33, 64} and {s[0] for s in wide} >= {1, 3, 4, 5, 15, 16, 17, 33}
    assert {s[3] * s[4] for s in wide} >= {272, 320, 496, 511} and (10, 32) in {s[3:5] for s in wide}
    assert {(64, 1), (9, 7), (73, 7)} <= {s[3:5] for s in C.SHAPES}
    assert {s[2] == 1 for s in wide} == {True, False}
    for n, pixels, m, j, d, terms in C.SHAPES:
        assert G.capsule_lds_bytes(j, d, 1)[0] <= G.CAPSULE_LDS_BYTES
        assert 4 * (d * (j * d | 1) + 16 * (j * d | 1) + 16 * d + terms * j) <= G.CAPSULE_LDS_BYTES
        assert n * pixels * m * j * d * 4 <= 4.5e6


@pytest.mark.parametrize("name", ["squash", "logits"])
def test_edge_cases_on_the_emulation_and_their_measured_yardstick(name):
    case = C.get(name)
    f32 = case.f32_errors()
    res = case.run(EmuBackend())
    errs = case.errors(res)
    assert set(f32) == set(errs) and {k[0] if isinstance(k, tuple) else k for _, _, k in errs.values()} == set(EDGE_F32_ERR[name])
    for label, (err, width, key) in errs.items():
        print(f"{name} {label}: fp32 rendition {f32[label]:.3e}, emulation {err:.3e}")
    for label, (err, width, key) in errs.items():
        assert f32[label] <= edge_f32(name, key), (label, f32[label])  # the yardstick is what the constants say
        assert f32[label] >= 0.5 * edge_f32(name, key), (label, f32[label])  # ... and they are not padded
        assert err <= edge_limit(name, key), (label, err)
    C.assert_same_bits(res, case.run(EmuBackend()))


def test_logit_cases_defeat_the_float32_simplifications():
    """What an fp32 accumulation of the agreement, fp32 logits, or the cancelling softmax backward would return lies
    outside the limits -- by more than a factor of ten, not by luck."""
    case = C.get("logits")
    refs = {c.label: c for c in case.checks}
    for label, got in case.simplified.items():
        chk = refs[label.split("/")[0]]
        err = C.vector_err(got, chk.ref, chk.width)[0]
        print(f"{label}: {err:.3e} against a limit of {edge_limit('logits', chk.key):.3e}")
        assert err > 10 * edge_limit("logits", chk.key), (label, err)


def test_the_measures_refuse_a_planted_defect():
    case = C.get("squash")
    res = case.run(EmuBackend())
    n, j, d = 5, 2 * len(C.SQUASH_Q), 16
    small = {k: v.copy() for k, v in res.items()}
    view = small["v"][C.GUARD:C.GUARD + n * j * d].reshape(n, j, d)
    view[2, 1] *= np.float32(1.001)  # the q = 1e-14 capsule, entries of 1e-17: invisible relative to the tensor's largest
    assert C.tensor_err(view, C.ref_route_fwd(case.bufs["uhat"].reshape(n, -1, j, d), case.bufs["coef"].reshape(-1, j))[1]) < 1e-7
    assert case.errors(small)["route_fwd.v@q=1e-14"][0] > 5e-4
    zero = {k: v.copy() for k, v in res.items()}
    zero["ds_head_gy"][C.GUARD + 3] = np.float32(1e-30)  # class 0 is the zero capsule
    with pytest.raises(AssertionError, match="exactly zero"):
        case.errors(zero)
    for where in (C.GUARD - 1, C.GUARD + n * j):
        canary = {k: v.copy() for k, v in res.items()}
        canary["y"][where] = np.nextafter(PU.SENT, np.float32(0))
        with pytest.raises(AssertionError, match="outside the contract"):
            case.errors(canary)
    pad = C.get(C.SHAPES[1])
    res = pad.run(EmuBackend())
    n, pixels, m, j, d, _ = C.SHAPES[1]
    res["dx"][int(pad.bufs["dpix"][0]) + m * d] = 0.0  # the first pad column behind a written row of dx
    with pytest.raises(AssertionError, match="outside the contract"):
        pad.errors(res)


def test_refusal_table_is_consistent_with_the_planner_rule():
    for entry, tag, change in C.REFUSALS:
        if not tag.startswith("lds_"):
            continue
        spec = dict(C.BASELINE[entry], **change)
        j, d = (spec["jd"] // spec["d"], spec["d"]) if entry == "caps_uhat_fwd" else (spec["j"], spec["d"])
        fwd, bwd = G.capsule_lds_bytes(j, d, 3)
        assert (fwd if entry == "caps_uhat_fwd" else bwd) > G.CAPSULE_LDS_BYTES and d <= 32 and j * d <= 512
    assert G.capsule_lds_bytes(32, 16, 3) == (35840, 67328)
    assert len({C.refusal_id(r) for r in C.REFUSALS}) == len(C.REFUSALS)


@pytest.mark.parametrize("classes,width,seed", C.MODEL_CASES)
def test_model_level_cases_on_the_emulation(classes, width, seed):
    alg, params, x, onehot = C.model_inputs(classes, width, seed)
    built = PU.build("CAPModel", C.MODEL_PATCH, C.MODEL_CHANNELS, classes, alg, EmuBackend(), with_eval=False)
    sess = built.ctx.session()
    PU.inject(sess, params)
    ct = PU.run_train_step(built, x, onehot, {})
    ref = EC.torch_capsule_step(params, x, onehot, classes, alg, True)
    assert ref["qmin"] > 1e-6, "pick another seed"
    assert min(float(p.abs().min()) for p in ref["pre"].values()) > EC.KINK_ZONE, "pick another seed"
    assert EC.product_relu_decisions(built, ct, ref["pre"]) == ({}, 0)
    assert np.abs(ct.value(built.y_conv).numpy() - ref["logits"]).max() < TOL_LOGIT
    for k, g in ref["grads"].items():
        assert np.abs(sess.get_gradient("nn_core/" + k) - g).max() / max(np.abs(g).max(), 1e-6) < TOL_GRAD, k
