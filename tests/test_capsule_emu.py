"""CPU: the capsule classifier (hypelcnn_amd/nnmodel/CAPModel.py) on the kernel emulation against
tests/golden/reference_capsule.* -- values the reference's own CAPModel.py produced under a float64 stand-in
(tests/golden/make_reference_capsule.py).  The emulation keeps float32 buffers, so values are held to the project's float32
limits (README "Correctness"): logits 1e-3 absolute, every gradient within 5e-4 of that tensor's largest entry."""
import json
import os

import numpy as np
import pytest

from hypelcnn_amd import graph as G
from hypelcnn_amd.common import common_nn_ops as cno
from tests import emu_capsule as EC
from tests import parity_util as PU
from tests.emu_backend import EmuBackend

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_LOGIT, TOL_GRAD = 1e-3, 5e-4


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "reference_capsule.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "reference_capsule.npz"))


TRAIN_CASES = ["k1_decoder_r3", "k3_plain_r2", "k1_k3_plain_r1"]
ALL_CASES = TRAIN_CASES + ["evaluation_r3"]


def _build(meta, case):
    c = meta["cases"][case]
    built = PU.build("CAPModel", c["patch"], c["channels"], c["classes"], c["algorithm_params"], EmuBackend())
    return c, built


def _inject(sess, params):
    for k, v in params.items():
        sess.set_variable(k, v)


def test_registry_resolves_the_plugin():
    from hypelcnn_amd.nnmodel.NNModel import NNModel
    model = cno.get_model_from_name("CAPModel")
    assert isinstance(model, NNModel) and type(model).__name__ == "CAPModel"


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_variable_names_shapes_and_order_equal_the_reference(fixture, case):
    meta, _ = fixture
    c, built = _build(meta, case)
    got = [(v.name, list(v.shape), v.trainable) for v in built.template.store.order]
    want = [(v["name"], v["shape"], v["trainable"]) for v in c["variables"]]
    assert got == want


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_training_step_equals_the_reference(fixture, case):
    meta, arrays = fixture
    c, built = _build(meta, case)
    params, x, onehot, grads = EC.load_fixture_case(meta, arrays, case)
    sess = built.ctx.session()
    _inject(sess, params)
    state_before = sess.state.clone()
    ct = PU.run_train_step(built, x, onehot, {})
    err = np.abs(ct.value(built.y_conv).numpy() - arrays[f"{case}/y_conv"]).max()
    assert err < TOL_LOGIT, err
    assert abs(ct.loss_value() - c["loss"]) < TOL_LOGIT * max(1.0, abs(c["loss"]))
    out = built.template.towers[0]
    assert c["has_decoder"] == c["algorithm_params"]["enable_decoding"]
    for name, (want, index) in grads.items():
        got = sess.get_gradient(name).reshape(-1)
        got = got[index] if index is not None else got
        scale = max(np.abs(want).max(), 1e-6)
        assert np.abs(got - want.reshape(-1)).max() / scale < TOL_GRAD, name
    assert len(grads) == sum(v["trainable"] for v in c["variables"])
    assert not np.array_equal(sess.state.numpy(), state_before.numpy()), "the training step moves the moving averages"
    assert out.is_training


def test_decoder_output_equals_the_reference_and_is_absent_when_off(fixture):
    meta, arrays = fixture
    c, built = _build(meta, "k1_decoder_r3")
    params, x, onehot, _ = EC.load_fixture_case(meta, arrays, "k1_decoder_r3")
    _inject(built.ctx.session(), params)
    ct = PU.run_train_step(built, x, onehot, {})
    node = built.train_tower.nodes[-1]
    assert isinstance(node, G.LinearNode) and node.branches[0].w.name == "nn_core/DigitCaps_layer/Decoder/fc3/weights"
    assert np.abs(ct.value(node.out).numpy() - arrays["k1_decoder_r3/decoded"]).max() < TOL_LOGIT
    # decoder off, and any evaluation tower: no reconstruction
    alg = dict(c["algorithm_params"], enable_decoding=False)
    model = cno.get_model_from_name("CAPModel")
    template = cno.Template("nn_core", model.create_tensor_graph, class_count=3)
    for training, a in ((True, alg), (False, c["algorithm_params"])):
        out = template(cno.ModelInputParams(x=cno.Placeholder("x", (3, 3), 6), y=cno.Placeholder("labels", None, 3),
                                            device_id="/gpu:0", is_training=training), algorithm_params=a)
        assert out.image_output is None
        assert not any(isinstance(n, G.LabelMaskNode) for n in out.tower.nodes)


def test_evaluation_tower_uses_batch_statistics_and_leaves_the_moving_averages(fixture):
    meta, arrays = fixture
    c, built = _build(meta, "evaluation_r3")
    params, x, _, _ = EC.load_fixture_case(meta, arrays, "evaluation_r3")
    sess = built.ctx.session()
    _inject(sess, params)
    before = sess.state.clone()
    y = PU.run_eval(built, x)
    assert np.abs(y - arrays["evaluation_r3/y_conv"]).max() < TOL_LOGIT
    assert np.array_equal(sess.state.numpy(), before.numpy()), "an evaluation tower must not write the moving averages"
    assert (y.argmax(1) == arrays["evaluation_r3/y_conv"].argmax(1)).all()


def test_emulation_twin_agrees_with_the_float64_restatement():
    """The two yardsticks of the GPU tests -- fixture-independent: emulation step vs torch float64 autograd."""
    alg = dict(iter_routing=3, conv_layer_kernel_size=3, primary_caps_kernel_size=3, feature_count=8,
               primary_capsule_count=3, digit_capsule_output_space=4, optimizer="AdamOptimizer", learning_rate=1e-4,
               learning_rate_decay_factor=0.96, learning_rate_decay_step=350, lrelu_alpha=0.18, enable_decoding=True)
    rng = np.random.default_rng(5)
    built = PU.build("CAPModel", 5, 6, 3, alg, EmuBackend())
    params = EC.init_params(5, 6, 3, alg, rng, True)
    sess = built.ctx.session()
    PU.inject(sess, params)
    x = rng.random((6, 5, 5, 6)).astype(np.float32)
    onehot = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 6)]
    ct = PU.run_train_step(built, x, onehot, {})
    ref = EC.torch_capsule_step(params, x, onehot, 3, alg, True)
    assert ref["qmin"] > 1e-6
    assert np.abs(ct.value(built.y_conv).numpy() - ref["logits"]).max() < TOL_LOGIT
    for k, g in ref["grads"].items():
        assert np.abs(sess.get_gradient("nn_core/" + k) - g).max() / max(np.abs(g).max(), 1e-6) < TOL_GRAD, k


def test_refusals_name_their_reason(monkeypatch):
    tower = G.Tower(G.VariableStore("t"), True)
    x = tower.placeholder("x", (5, 5), 4)
    with pytest.raises(NotImplementedError, match="even kernel"):
        G.conv2d(x, 8, [2, 2], scope="c", padding="VALID")
    assert G.conv2d(x, 8, [3, 3], scope="c3", padding="VALID").hw == (3, 3)
    assert G.conv2d(x, 8, [1, 1], scope="c1", padding="VALID").hw == (5, 5)
    with pytest.raises(NotImplementedError, match="routing kernels"):
        G.capsule_routing(G.conv2d(x, 2 * 64, [1, 1], scope="wide"), 2, 3, 64, 3)

    def route(training, classes, width, iterations=3):
        t = G.Tower(G.VariableStore("t"), training)
        return G.capsule_routing(G.conv2d(t.placeholder("x", (1, 1), 4), width, [1, 1], scope="c"), 1, classes, width, iterations)

    # the LDS of the two u_hat products (include/hypel.h "Limits"): corner shapes that pass the width / column limits
    for classes, width in ((32, 16), (11, 32), (15, 32), (16, 32)):
        with pytest.raises(NotImplementedError, match=r"bytes of LDS per block.*65536-byte limit"):
            route(True, classes, width)
    with pytest.raises(NotImplementedError, match="67328"):
        route(True, 32, 16)
    with pytest.raises(NotImplementedError, match="LDS"):
        route(True, 31, 16, iterations=5)  # the backward's 2R-1 coefficient rows count too
    with pytest.raises(NotImplementedError, match="evaluation tower needs the forward product only"):
        route(False, 16, 32)
    for training, classes, width in ((True, 31, 16), (True, 10, 32), (True, 20, 16), (False, 32, 16), (False, 11, 32),
                                     (False, 15, 32)):
        assert route(training, classes, width)[1].c == classes * width
    assert route(True, 31, 16, iterations=4)[0].c == 31
    monkeypatch.setenv("WORLD_SIZE", "2")
    alg = dict(iter_routing=1, conv_layer_kernel_size=1, primary_caps_kernel_size=1, feature_count=4, primary_capsule_count=2,
               digit_capsule_output_space=4, lrelu_alpha=0.1, enable_decoding=False)
    with pytest.raises(NotImplementedError, match="data parallel"):
        cno.get_model_from_name("CAPModel").create_tensor_graph(
            cno.ModelInputParams(x=x, y=None, device_id="/gpu:0", is_training=True), 3, alg)
    monkeypatch.delenv("WORLD_SIZE")
    from hypelcnn_amd import tf_facade
    with pytest.raises(NotImplementedError, match="facade"):
        tf_facade.reference_model("CAPModel", "/nonexistent")


def test_planner_refuses_a_batch_beyond_the_routing_grid():
    alg = dict(iter_routing=2, conv_layer_kernel_size=1, primary_caps_kernel_size=1, feature_count=2, primary_capsule_count=1,
               digit_capsule_output_space=2, optimizer="AdamOptimizer", learning_rate=1e-4, learning_rate_decay_factor=0.96,
               learning_rate_decay_step=350, lrelu_alpha=0.1, enable_decoding=False)
    built = PU.build("CAPModel", 1, 2, 2, alg, EmuBackend())
    built.ctx.session()
    assert G.CAPSULE_MAX_BATCH == 65535
    with pytest.raises(NotImplementedError, match="batch of 65536 exceeds the 65535"):
        built.train_step.compiled(65536)
    with pytest.raises(NotImplementedError, match="batch of 65536 exceeds the 65535"):
        PU.run_eval(built, np.zeros((65536, 1, 1, 2), np.float32))
    built.train_step.compiled(65535)


def test_capsule_fits_never_admits_what_the_kernels_refuse():
    """(J, D, R) over the whole admitted domain against the formulas as include/hypel.h documents them: what the Python
    rule admits fits the 64 KB, and what it refuses inside the width / column limits does not (the rule is the kernels',
    not a narrower one)."""
    cap = 64 * 1024
    admitted = refused = 0
    for d in range(1, 33):
        for j in range(1, 512 // d + 1):
            jd = j * d
            fwd = 4 * ((d + 1) * jd + 16 * d)
            for r in range(1, 9):
                jdp, terms = jd | 1, 2 * r - 1
                bwd = 4 * (d * jdp + 16 * jdp + 16 * d + terms * j)
                assert G.capsule_lds_bytes(j, d, r) == (fwd, bwd)
                assert G.capsule_fits(j, d, r, False) == (fwd <= cap)
                assert G.capsule_fits(j, d, r, True) == (fwd <= cap and bwd <= cap)
                admitted += G.capsule_fits(j, d, r, True)
                refused += not G.capsule_fits(j, d, r, True)
    assert admitted > 10000 and refused > 100
    assert not G.capsule_fits(1, 33, 1, False) and not G.capsule_fits(513, 1, 1, False) and not G.capsule_fits(2, 2, 0, False)
    import re
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "hypel.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define\s+HYPEL_CAPS_MAX_(\w+)\s+(\d+)", header)}
    assert limits == dict(D=G.CAPSULE_MAX_WIDTH, JD=G.CAPSULE_MAX_COLS, N=G.CAPSULE_MAX_BATCH, LDS=G.CAPSULE_LDS_BYTES)
    # the corners the header names
    assert G.capsule_fits(31, 16, 4, True) and not G.capsule_fits(31, 16, 5, True) and not G.capsule_fits(32, 16, 1, True)
    assert G.capsule_fits(10, 32, 3, True) and not G.capsule_fits(11, 32, 1, True)
    assert G.capsule_fits(32, 16, 3, False) and G.capsule_fits(15, 32, 3, False) and not G.capsule_fits(16, 32, 3, False)


def test_planner_refuses_a_data_parallel_session(fixture):
    meta, _ = fixture
    c, built = _build(meta, "k3_plain_r2")
    sess = built.ctx.session()
    sess.dist = (2, 0)
    with pytest.raises(NotImplementedError, match="all-reduce inside every routing iteration"):
        built.train_step.compiled(4)


def test_checkpoint_round_trip_keeps_the_reference_key_names(fixture, tmp_path):
    from hypelcnn_amd.classify import monitored_session_runner as M
    from hypelcnn_amd.common import tf_checkpoint as T
    meta, arrays = fixture
    c, b1 = _build(meta, "k1_decoder_r3")
    params, x, onehot, _ = EC.load_fixture_case(meta, arrays, "k1_decoder_r3")
    s1 = b1.ctx.session()
    _inject(s1, params)
    for _ in range(2):
        PU.run_train_step(b1, x, onehot, {})
        s1.adam_step(1e-3)
    prefix = M.export_tf_checkpoint(s1, str(tmp_path / "model.ckpt-2"))
    names = set(T.read_index(prefix + ".index"))
    assert {b"nn_core/Conv1_layer/weights", b"nn_core/PrimaryCaps_layer/BatchNorm/moving_variance",
            b"nn_core/DigitCaps_layer/DigitCaps_layer_w_0/weights", b"nn_core/DigitCaps_layer/DigitCaps_layer_w_26/biases",
            b"nn_core/DigitCaps_layer/Decoder/fc1/weights",
            b"nn_core/DigitCaps_layer/DigitCaps_layer_w_3/weights/nn_core/Adam_1"} <= names
    stored = T.read_checkpoint(prefix, names={"nn_core/DigitCaps_layer/DigitCaps_layer_w_5/weights"})
    assert stored["nn_core/DigitCaps_layer/DigitCaps_layer_w_5/weights"].shape == (1, 1, 4, 12)
    _, b2 = _build(meta, "k1_decoder_r3")
    s2 = b2.ctx.session()
    M.restore_checkpoint(s2, prefix)
    np.testing.assert_array_equal(s2.params.numpy(), s1.params.numpy())
    np.testing.assert_array_equal(s2.state.numpy(), s1.state.numpy())
    for b, s in ((b1, s1), (b2, s2)):
        PU.run_train_step(b, x, onehot, {})
        s.adam_step(1e-3)
    np.testing.assert_array_equal(s2.params.numpy(), s1.params.numpy())


def test_capsule_weights_form_one_slab():
    alg = dict(iter_routing=2, conv_layer_kernel_size=1, primary_caps_kernel_size=1, feature_count=4, primary_capsule_count=2,
               digit_capsule_output_space=4, optimizer="AdamOptimizer", learning_rate=1e-4, learning_rate_decay_factor=0.96,
               learning_rate_decay_step=350, lrelu_alpha=0.1, enable_decoding=True)
    built = PU.build("CAPModel", 3, 5, 3, alg, EmuBackend())
    built.ctx.session()
    node = next(n for n in built.train_tower.nodes if isinstance(n, G.CapsuleNode))
    assert node.capsules == 18
    for vs in (node.weights, node.biases):
        assert all(b.offset == a.offset + a.size for a, b in zip(vs, vs[1:]))
