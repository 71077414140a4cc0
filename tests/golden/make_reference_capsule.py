#!/usr/bin/env python3
"""Pin the capsule classifier by executing the reference's own text (build container only; needs /root/reference).

`nnmodel/CAPModel.py` runs UNCHANGED -- `create_tensor_graph` and the public `get_loss_func` -- under the numeric float64
stand-in of `capsule_standin.py`.  Written to tests/golden/reference_capsule.json / .npz per case: the variable names and
shapes in creation order, the inputs, every variable's value, y_conv, the decoder output, the loss reduced as
`optimize_nn` reduces it (mean over the per-sample vector), and the gradient of that loss for every trainable variable.
All values are fp32-representable.  To keep the file small, a variable above 262 144 elements (the decoder's 512 x 1024
matrix) is stored as the (seed, limit) of `tests/emu_capsule.hashed_uniform` and its gradient as every 61st element;
gradients above 16 384 elements are stored as float32.  The script fails if any squash argument q falls below 1e-6.  Data only."""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference"

import capsule_standin as S  # noqa: E402
from tests.emu_capsule import FIXTURE_GENERATED_ABOVE, FIXTURE_GRAD_STRIDE, hashed_uniform  # noqa: E402

BASE = dict(feature_count=8, primary_capsule_count=3, primary_capsule_output_space=8, digit_capsule_output_space=4,
            batch_size=5, optimizer="AdamOptimizer", learning_rate=1e-4, learning_rate_decay_factor=0.96,
            learning_rate_decay_step=350, lrelu_alpha=0.18)
# (case, training, patch, channels, classes, batch, overrides)
CASES = [
    ("k1_decoder_r3", True, 3, 6, 3, 5, dict(conv_layer_kernel_size=1, primary_caps_kernel_size=1, enable_decoding=True, iter_routing=3)),
    ("k3_plain_r2", True, 5, 7, 4, 5, dict(conv_layer_kernel_size=3, primary_caps_kernel_size=1, enable_decoding=False, iter_routing=2)),
    ("k1_k3_plain_r1", True, 5, 6, 3, 5, dict(conv_layer_kernel_size=1, primary_caps_kernel_size=3, enable_decoding=False, iter_routing=1)),
    ("evaluation_r3", False, 3, 6, 3, 5, dict(conv_layer_kernel_size=1, primary_caps_kernel_size=1, enable_decoding=True, iter_routing=3)),
]

Q_SEEN = []


def _watch_squash():
    """The plugin computes q with tf.reduce_mean(tf.square(s_j), axis=1, keepdims=True): record the smallest value."""
    import tensorflow as tf
    inner = tf.reduce_mean

    def reduce_mean(input_tensor, axis=None, keepdims=False):
        out = inner(input_tensor=input_tensor, axis=axis, keepdims=keepdims)
        if keepdims and axis == 1:
            Q_SEEN.append(float(out.t.detach().min()))
        return out
    tf.reduce_mean = reduce_mean


def fp32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def run_case(model_cls, ops, name, training, patch, channels, classes, batch, alg, seed):
    rng = np.random.default_rng(seed)
    x = fp32(rng.random((batch, patch, patch, channels)))
    onehot = np.eye(classes)[rng.integers(0, classes, batch)]

    def build(preset):
        S.STORE[0] = S.Store(np.random.default_rng(seed + 1), preset)
        model = model_cls()
        mip = ops.ModelInputParams(x=S.T(torch.tensor(x, dtype=S.DT)), y=S.T(torch.tensor(onehot, dtype=S.DT)),
                                   device_id="/cpu:0", is_training=training)
        with S.variable_scope("nn_core"):
            out = model.create_tensor_graph(mip, classes, alg)
        return model, out

    # first pass: learn the variable list; then give every variable a non-trivial fp32-representable value
    build(None)
    first = S.STORE[0]
    preset, generated = {}, {}
    for k, n in enumerate(first.order):
        v = first.vars[n].detach().numpy()
        if n.endswith(("biases", "beta")):
            v = rng.standard_normal(v.shape) * 0.05 + (0.2 if n.endswith("beta") else 0.0)
        elif n.endswith("moving_mean"):
            v = rng.standard_normal(v.shape) * 0.1
        elif n.endswith("moving_variance"):
            v = rng.random(v.shape) + 0.5
        if v.size > FIXTURE_GENERATED_ABOVE:
            lim = float(np.sqrt(6.0 / (v.shape[-2] + v.shape[-1])))
            generated[n] = dict(seed=seed * 1000 + k, limit=lim)
            v = hashed_uniform(v.size, generated[n]["seed"], lim).reshape(v.shape)
        preset[n] = fp32(v)
    Q_SEEN.clear()
    model, out = build(preset)
    st = S.STORE[0]
    assert st.order == first.order
    assert min(Q_SEEN) > 1e-6, f"{name}: squash argument {min(Q_SEEN)} too small to compare gradients at"
    meta = {"training": training, "patch": patch, "channels": channels, "classes": classes, "batch": batch,
            "algorithm_params": alg, "min_q": min(Q_SEEN), "variables": []}
    arrays = {f"{name}/x": x.astype(np.float32), f"{name}/onehot": onehot.astype(np.float32),
              f"{name}/y_conv": out.y_conv.t.detach().numpy()}
    meta["has_decoder"] = out.image_output is not None
    if out.image_output is not None:
        arrays[f"{name}/decoded"] = out.image_output.t.detach().numpy()
    grads = {}
    if training:
        per_sample = model.get_loss_func(out, S.T(torch.tensor(onehot, dtype=S.DT)))
        loss = per_sample.t.mean()  # optimize_nn: tf.reduce_mean(loss_func(...)) (common/common_nn_ops.py:214)
        meta["loss"] = float(loss.detach())
        names = [n for n in st.order if st.trainable[n]]
        grads = dict(zip(names, torch.autograd.grad(loss, [st.vars[n] for n in names])))
    for n in st.order:
        v = st.vars[n].detach().numpy()
        rec = {"name": n, "shape": list(v.shape), "trainable": bool(st.trainable[n])}
        if n in generated:
            rec["generated"] = generated[n]
        else:
            arrays[f"{name}/value/{n}"] = v.astype(np.float32)
        if n in grads:
            g = grads[n].numpy()
            if n in generated:
                rec["grad_stride"] = FIXTURE_GRAD_STRIDE
                rec["grad_max"] = float(np.abs(g).max())
                g = g.reshape(-1)[::FIXTURE_GRAD_STRIDE]
            elif g.size > 16384:
                g = g.astype(np.float32)
            arrays[f"{name}/grad/{n}"] = g
        meta["variables"].append(rec)
    return meta, arrays


def main():
    if not os.path.isdir(REF):
        raise SystemExit("the reference is only present in the build container")
    S.install()
    sys.path.insert(0, REF)
    _watch_squash()
    mod = importlib.import_module("nnmodel.CAPModel")
    assert os.path.abspath(mod.__file__).startswith(REF + os.sep)
    ops = sys.modules["common.common_nn_ops"]
    meta, arrays = {"cases": {}}, {}
    for k, (name, training, patch, channels, classes, batch, over) in enumerate(CASES):
        m, a = run_case(mod.CAPModel, ops, name, training, patch, channels, classes, batch, dict(BASE, **over), 100 + k)
        meta["cases"][name] = m
        arrays.update(a)
        print(name, "min q", m["min_q"], "loss", m.get("loss"), "variables", len(m["variables"]))
    with open(os.path.join(HERE, "reference_capsule.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "reference_capsule.npz"), **arrays)


if __name__ == "__main__":
    main()
