#!/usr/bin/env python3
"""Record what the REFERENCE's own files produce through the product's facades (build container only; needs /root/reference).

The facades (`hypelcnn_amd.tf_facade.reference_model`, `hypelcnn_amd.tfgan_facade.reference_wrapper`) run the reference's
unchanged plugin and wrapper files onto the product's graph.  This script runs them once and writes what came out, as data,
to tests/golden/reference_facade.json / .npz, so that the tests hold the product to it on any machine:

  * classifiers: for three small configurations, the training and inference Towers the reference's plugin file records and
    the gradients of one training step on the kernel emulation (tests/test_reference_wiring.py);
  * GAN wrappers: per case of reference_gan_wiring.json, the phases the reference's wrapper files define (names, terms with
    operands by provenance, weights, trained groups, LR schedule, tensor-pool feeds, variables; tests/test_reference_gan_wiring.py);
  * `gan/gan_train_for_shadow.py::perform_shadow_augmentation_random` with its two uniform draws pinned, for five draw pairs;
  * the reference's CycleGAN inference wrapper used as an augmenter on a [P, P, B + 1] patch, in float64, both directions
    (tests/test_reference_optimize.py).

Each part runs in a fresh interpreter (the stand-ins install process-wide import hooks).  Re-running this script and
finding no change under `git diff tests/golden` is the check that the fixture is current.  Data only."""
import json
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

# (case, model, patch, channels, classes, algorithm params, batch)
CLASSIFIER_CASES = [
    ("hypelcnn", "HYPELCNNModel", 5, 11, 4, {"drop_out_ratio": 0.7, "filter_count": 48, "learning_rate": 3e-4,
                                             "learning_rate_decay_factor": 0.96, "learning_rate_decay_step": 350,
                                             "lrelu_alpha": 0.18, "optimizer": "AdamOptimizer", "bn_decay": 0.95,
                                             "l2regularizer_scale": 1e-5, "spectral_hierarchy_level": 3,
                                             "spatial_hierarchy_level": 3, "degradation_coeff": 3, "use_residual": True,
                                             "batch_size": 6}, 6),
    ("dualcnn", "DUALCNNModel", 5, 7, 3, {"drop_out_ratio": 0.7, "lrelu_alpha": 0.18, "filter_count": 32, "hs_lidar_diff": 1,
                                          "optimizer": "AdamOptimizer", "learning_rate": 3e-4,
                                          "learning_rate_decay_factor": 0.96, "learning_rate_decay_step": 350}, 4),
    ("concnn", "CONCNNModel", 5, 9, 3, {"drop_out_ratio": 0.5, "filter_count": 6, "optimizer": ["MomentumOptimizer", 0.9],
                                        "learning_rate": 1e-3, "learning_rate_decay_factor": 0.01,
                                        "learning_rate_decay_step": 33333}, 4),
]
SHADOW_DRAWS = [(0.1, 0.1), (0.1, 0.9), (0.9, 0.1), (0.9, 0.9), (0.4, 0.39999)]


def classifier_tower(model_name, patch, ch, classes, alg, is_training, model=None):
    """The Tower a plugin records (the product's own when `model` is None), as graph_dump describes it."""
    sys.path.insert(0, HERE)
    from graph_dump import dump_output, dump_store, dump_tower
    from hypelcnn_amd import graph as G
    from hypelcnn_amd.common import common_nn_ops as P
    model = model or P.get_model_from_name(model_name)
    store = G.VariableStore("nn_core")
    tower = G.Tower(store, is_training)
    x = tower.placeholder("x", (patch, patch), ch)
    out = model.create_tensor_graph(P.ModelInputParams(x=x, y=None, device_id="/gpu:0", is_training=is_training),
                                    classes, alg)
    return json.loads(json.dumps({"tower": dump_tower(tower), "variables": dump_store(store),
                                  "y_conv": dump_output(out.y_conv),
                                  "image_output": None if out.image_output is None else dump_output(out.image_output)}))


def classifier_gradients(model_name, patch, ch, classes, alg, nb, model=None):
    """One training step on the kernel emulation (the product's plugin when `model` is None), checked against the oracle:
    every trainable variable's gradient, concatenated in sorted name order."""
    from tests import parity_util as U
    from tests.emu_backend import EmuBackend
    rng = np.random.default_rng(3)
    built = U.build(model_name, patch, ch, classes, alg, EmuBackend(), model=model)
    sess = built.ctx.session()
    params = U.make_params(model_name, patch, ch, classes, alg, rng)
    U.inject(sess, params)
    x = rng.random((nb, patch, patch, ch)).astype(np.float32)
    onehot = np.eye(classes, dtype=np.float32)[rng.integers(0, classes, nb)]
    masks = U.make_masks(built, nb, rng)
    ct = U.run_train_step(built, x, onehot, masks)
    U.compare_step(built, ct, params, x, onehot, masks, model_name, classes, alg, tol_logit=2e-5, tol_grad=2e-4)
    return np.concatenate([np.asarray(sess.get_gradient("nn_core/" + k), np.float32).ravel() for k in sorted(params)])


def gan_phases_jsonable(phases_and_vars, use_pool):
    """`tests/test_reference_gan_wiring.py::_canonical_phases` output in a JSON round-trippable form."""
    phases, variables = phases_and_vars
    out = []
    for p in phases:
        terms = sorted(([list(k), w] for k, w in p["terms"].items()), key=repr)
        out.append(dict(p, terms=terms, pool=[list(q) for q in p["pool"]]))
    return json.loads(json.dumps({"phases": out, "variables": [list(v) for v in variables], "use_pool": use_pool}))


# ------------------------------------------------------------------------------------------------ the parts (one process each)
def part_classifiers():
    from hypelcnn_amd import tf_facade
    js, arr = {}, {}
    for name, model_name, patch, ch, classes, alg, nb in CLASSIFIER_CASES:
        ref = tf_facade.reference_model(model_name, REF)
        js[name] = {"model": model_name, "patch": patch, "channels": ch, "classes": classes, "alg": alg, "batch": nb,
                    "towers": {mode: classifier_tower(model_name, patch, ch, classes, alg, training, model=ref)
                               for mode, training in (("train", True), ("eval", False))}}
        arr[f"{name}/gradients"] = classifier_gradients(model_name, patch, ch, classes, alg, nb, model=ref)
    return js, arr


def part_gan_phases():
    from types import SimpleNamespace
    from hypelcnn_amd import tfgan_facade
    from hypelcnn_amd.gan.wrappers import gan_common as C
    from tests import test_reference_gan_wiring as T
    from tests.emu_backend import EmuBackend
    js = {}
    for case in T.CASES:
        c = T.FIX[case]
        f = c["flags"]
        wrapper = tfgan_facade.reference_wrapper(c["gan_type"], REF, SimpleNamespace(**f))
        wrapper.backend = EmuBackend()
        tower, x, y = C.new_gan_tower(c["bands"])
        model = wrapper.define_model(x, y)
        loss = wrapper.define_loss(model)
        ops = wrapper.define_train_ops(model, loss, max_number_of_steps=c["max_steps"], generator_lr=f["generator_lr"],
                                       discriminator_lr=f["discriminator_lr"], gen_discriminator_lr=f["gen_discriminator_lr"])
        js[case] = gan_phases_jsonable(T._canonical_phases(ops.loss, ops, c), bool(ops.use_pool))
    return js, {}


def part_shadow_augmentation():
    sys.path.insert(0, HERE)
    import importlib
    import tf_standin as S
    from hypelcnn_amd import tf_facade as F
    from hypelcnn_amd import tfgan_facade as TG
    draws = []

    def _setup(m):
        if m.__name__ == "tensorflow":
            m.less = lambda a, b: a < b
            m.cond = lambda pred=None, true_fn=None, false_fn=None, **k: true_fn() if pred else false_fn()
            m.device = F._Ctx
        elif m.__name__ == "tensorflow.random":
            m.uniform = lambda shape, lo, hi, **k: [draws.pop(0)]
        elif m.__name__ == "tensorflow.compat.v1":
            m.name_scope = F._Ctx
    TG.enable()                                  # the module imports the wrapper registry (the tensorflow_gan surface)
    F._Finder.EXTRA_SETUP.append(_setup)         # after it: this part's eager tf.cond wins
    S.install()
    TG.preload()
    tf = importlib.import_module("tensorflow")
    tf.random = importlib.import_module("tensorflow.random")
    ref = importlib.import_module("gan.gan_train_for_shadow")
    rng = np.random.default_rng(3)
    bands, rate = 7, 0.4
    normal = rng.random(bands).astype(np.float32)
    shadow = (rng.random(bands) * 0.5).astype(np.float32)
    ratio = (1.5 + rng.random(bands)).astype(np.float32)
    arr = {"normal": normal, "shadow": shadow, "ratio": ratio, "draws": np.float32(SHADOW_DRAWS)}
    xs, ys = [], []
    for u1, u2 in SHADOW_DRAWS:
        draws[:] = [u1, u2]
        x_ref, y_ref = ref.perform_shadow_augmentation_random(normal.copy(), shadow.copy(), ratio, rate)
        xs.append(np.asarray(x_ref, np.float32))
        ys.append(np.asarray(y_ref, np.float32))
    arr["x"], arr["y"] = np.stack(xs), np.stack(ys)
    return {"rate": rate}, {"shadow_aug/" + k: v for k, v in arr.items()}


def part_generator_augmenter():
    sys.path.insert(0, HERE)
    import importlib
    import tfgan_standin as W
    W.install()
    util = importlib.import_module("gan.gan_utilities")
    registry = importlib.import_module("gan.wrapper_registry")
    P, B = 3, 16
    rng = np.random.default_rng(11)
    patch = rng.random((P, P, B + 1))
    holder = util.create_gan_struct(registry.get_infer_wrapper_dict()["cycle_gan"], "", "")
    eng = W.WiringEngine(rng=np.random.default_rng(12))
    with W.S.use_engine(eng):
        t = eng.placeholder(patch, "patch")
        shadow_out = np.asarray(holder.shadow_op(t).var.v, np.float64)
        deshadow_out = np.asarray(holder.deshadow_op(t).var.v, np.float64)
    arr = {"gen_aug/patch": patch, "gen_aug/shadow": shadow_out, "gen_aug/deshadow": deshadow_out}
    for k, v in eng.params.items():
        arr["gen_aug/param/" + k] = np.asarray(v, np.float64)
    return {"variables": sorted(eng.variables), "P": P, "B": B}, arr


PARTS = {"classifiers": part_classifiers, "gan_phases": part_gan_phases, "shadow_augmentation": part_shadow_augmentation,
         "generator_augmenter": part_generator_augmenter}


def main():
    if len(sys.argv) == 3:                       # one part, in this (fresh) interpreter
        sys.path.insert(0, ROOT)
        js, arr = PARTS[sys.argv[1]]()
        with open(sys.argv[2], "wb") as f:
            pickle.dump((js, arr), f)
        return
    if not os.path.isdir(REF):
        raise SystemExit("needs the reference checkout")
    js, arr = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for part in PARTS:
            out = os.path.join(tmp, part + ".pkl")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), part, out], cwd=ROOT)
            with open(out, "rb") as f:
                j, a = pickle.load(f)
            js[part] = j
            arr.update(a)
    with open(os.path.join(HERE, "reference_facade.json"), "w") as f:
        json.dump(js, f, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "reference_facade.npz"), **arr)
    print("wrote", sorted(js), len(arr), "arrays")


if __name__ == "__main__":
    main()
