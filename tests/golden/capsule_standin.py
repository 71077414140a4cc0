"""Numeric float64 stand-in for the `tensorflow` / `tf_slim` names the reference's capsule plugin imports (build container
only).  TEST INFRASTRUCTURE.

Unlike `tf_standin.py` (which records layer calls or routes them into the product's graph), this one EVALUATES: every
`tf.*` / `tf_slim.*` call the plugin makes returns a tensor holding a torch float64 value with autograd, so the plugin's
own per-capsule Python loop of split / tile / depthwise_conv2d / matmul produces numbers and gradients.  tf_slim's defaults
are restated here: `conv2d` / `fully_connected` use ReLU, Xavier-uniform weights and zero biases, a normaliser replaces the
bias, and `batch_norm(is_training=True, decay=0.999, epsilon=0.001, center=True, scale=False)` normalises with the biased
statistics of the batch in hand.  Variables are created once per name (creation order is recorded) and may be preset.
"""
import contextlib
import math
import sys
import types

import numpy as np
import torch

DT = torch.float64


class Dim(int):
    """tf Dimension: multiplies to a Dimension, has `.value`."""

    @property
    def value(self):
        return int(self)

    def __mul__(self, other):
        return Dim(int(self) * int(other))

    __rmul__ = __mul__


def _raw(v):
    return v.t if isinstance(v, T) else v


class T:
    """A tensor of the stand-in: `.t` is the torch value."""

    def __init__(self, t):
        self.t = t

    def get_shape(self):
        return [Dim(s) for s in self.t.shape]

    shape = property(get_shape)

    def __add__(self, o):
        return T(self.t + _raw(o))

    __radd__ = __add__

    def __sub__(self, o):
        return T(self.t - _raw(o))

    def __rsub__(self, o):
        return T(_raw(o) - self.t)

    def __mul__(self, o):
        return T(self.t * _raw(o))

    __rmul__ = __mul__

    def __truediv__(self, o):
        return T(self.t / _raw(o))


class Store:
    """Variables by full name, in creation order; `preset` values win over the initialisers."""

    def __init__(self, rng, preset=None):
        self.rng = rng
        self.preset = dict(preset or {})
        self.vars = {}
        self.order = []
        self.trainable = {}

    def get(self, name, shape, init, trainable=True):
        if name not in self.vars:
            if name in self.preset:
                val = np.asarray(self.preset[name], np.float64).reshape(shape)
            else:
                val = init(self.rng, shape)
            self.vars[name] = torch.tensor(val, dtype=DT, requires_grad=trainable)
            self.order.append(name)
            self.trainable[name] = trainable
        assert tuple(self.vars[name].shape) == tuple(shape), (name, shape)
        return self.vars[name]


STORE = [None]
_SCOPES = [""]
_ARGS = [{}]


class Scope:
    def __init__(self, full):
        self.name = full


@contextlib.contextmanager
def variable_scope(name_or_scope, default_name=None, values=None, reuse=None):
    if isinstance(name_or_scope, Scope):
        full = name_or_scope.name  # re-entering a captured scope does not nest
    else:
        full = (_SCOPES[-1] + "/" + name_or_scope) if _SCOPES[-1] else name_or_scope
    _SCOPES.append(full)
    try:
        yield Scope(full)
    finally:
        _SCOPES.pop()


def _var(name, shape, init, trainable=True):
    return STORE[0].get(_SCOPES[-1] + "/" + name, tuple(int(s) for s in shape), init, trainable)


def _xavier(rng, shape):
    rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    lim = math.sqrt(6.0 / ((shape[-2] + shape[-1]) * rf))
    return rng.uniform(-lim, lim, shape)


def _zeros(rng, shape):
    return np.zeros(shape)


def _ones(rng, shape):
    return np.ones(shape)


# ------------------------------------------------------------------------------------------------- tf_slim
@contextlib.contextmanager
def arg_scope(funcs, **kwargs):
    merged = dict(_ARGS[-1])
    for f in funcs:
        merged[f.__name__] = dict(merged.get(f.__name__, {}), **kwargs)
    _ARGS.append(merged)
    try:
        yield
    finally:
        _ARGS.pop()


def _with_arg_scope(fn):
    def wrapped(*a, **kw):
        merged = dict(_ARGS[-1].get(fn.__name__, {}))
        merged.update(kw)
        return fn(*a, **merged)
    wrapped.__name__ = fn.__name__
    return wrapped


def relu(x):
    return T(torch.relu(_raw(x)))


@_with_arg_scope
def batch_norm(inputs, decay=0.999, center=True, scale=False, epsilon=0.001, is_training=True, scope=None, trainable=True):
    assert center and not scale
    with variable_scope(scope or "BatchNorm"):
        c = inputs.t.shape[-1]
        beta = _var("beta", (c,), _zeros, trainable)
        mm = _var("moving_mean", (c,), _zeros, False)
        mv = _var("moving_variance", (c,), _ones, False)
    x = inputs.t
    if is_training:
        axes = tuple(range(x.dim() - 1))
        mean = x.mean(axes)
        var = ((x - mean) ** 2).mean(axes)
    else:
        mean, var = mm, mv
    return T((x - mean) / torch.sqrt(var + epsilon) + beta)


def _finish(y, num_outputs, activation_fn, normalizer_fn, normalizer_params, trainable):
    if normalizer_fn is not None:
        y = normalizer_fn(y, **(normalizer_params or {}))
    else:
        y = T(y.t + _var("biases", (num_outputs,), _zeros, trainable))
    return activation_fn(y) if activation_fn is not None else y


@_with_arg_scope
def conv2d(inputs, num_outputs, kernel_size, stride=1, padding="SAME", activation_fn=relu, normalizer_fn=None,
           normalizer_params=None, trainable=True, scope=None):
    kh, kw = (kernel_size, kernel_size) if isinstance(kernel_size, int) else kernel_size
    assert stride == 1 and padding == "VALID", "the capsule plugin only uses stride 1, VALID"
    with variable_scope(scope if scope is not None else "Conv"):
        cin = inputs.t.shape[-1]
        w = _var("weights", (kh, kw, cin, num_outputs), _xavier, trainable)
        y = torch.nn.functional.conv2d(inputs.t.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1)).permute(0, 2, 3, 1)
        return _finish(T(y), num_outputs, activation_fn, normalizer_fn, normalizer_params, trainable)


@_with_arg_scope
def fully_connected(inputs, num_outputs, activation_fn=relu, normalizer_fn=None, normalizer_params=None, trainable=True,
                    scope=None):
    with variable_scope(scope if scope is not None else "fully_connected"):
        w = _var("weights", (inputs.t.shape[-1], num_outputs), _xavier, trainable)
        return _finish(T(inputs.t @ w), num_outputs, activation_fn, normalizer_fn, normalizer_params, trainable)


# ------------------------------------------------------------------------------------------------- tensorflow
def _ints(shape):
    return [int(s) for s in shape]


def reshape(tensor, shape):
    return T(_raw(tensor).reshape(_ints(shape)))


def split(value, num_or_size_splits, axis=0):
    t = _raw(value)
    n = int(num_or_size_splits)
    return [T(p) for p in torch.split(t, t.shape[axis] // n, dim=axis)]


def concat(values, axis):
    return T(torch.cat([_raw(v) for v in values], dim=axis))


def constant(value, dtype=None):
    return T(torch.tensor(np.asarray(value), dtype=DT))


def tile(tensor, multiples):
    return T(_raw(tensor).repeat(*_ints(multiples)))


def softmax(logits, axis=-1):
    return T(torch.softmax(_raw(logits), dim=axis))


def depthwise_conv2d(input, filter, strides, padding):  # noqa: A002 (TensorFlow's parameter names)
    """NHWC input [N, H, W, C], filter [fh, fw, C, multiplier]; stride 1, VALID."""
    x, f = _raw(input), _raw(filter)
    assert list(strides) == [1, 1, 1, 1] and padding == "VALID"
    fh, fw, c, mult = f.shape
    w = f.permute(2, 3, 0, 1).reshape(c * mult, 1, fh, fw)
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, groups=c)
    return T(y.permute(0, 2, 3, 1))


def _reduce(fn):
    def op(input_tensor, axis=None, keepdims=False):
        t = _raw(input_tensor)
        return T(fn(t) if axis is None else fn(t, dim=axis, keepdim=keepdims))
    return op


def matmul(a, b, transpose_a=False, transpose_b=False):
    a, b = _raw(a), _raw(b)
    if transpose_a:
        a = a.transpose(-1, -2)
    if transpose_b:
        b = b.transpose(-1, -2)
    return T(a @ b)


def norm(tensor, axis=None):
    t = _raw(tensor)
    return T(torch.sqrt((t * t).sum(dim=axis)))


def softmax_cross_entropy_with_logits(labels, logits):
    return T(-(_raw(labels) * torch.log_softmax(_raw(logits), dim=-1)).sum(-1))


def leaky_relu(features, alpha=0.2):
    t = _raw(features)
    return T(torch.where(t > 0, t, t * alpha))


def install():
    """Serve `tensorflow`, `tensorflow.python.ops.gen_nn_ops`, `tf_slim` and the two small modules of the reference the
    plugin imports value classes from.  Returns the names it put into sys.modules."""
    tf = types.ModuleType("tensorflow")
    tf.float32 = "float32"
    tf.device = lambda name: contextlib.nullcontext()
    tf.reshape, tf.split, tf.concat, tf.constant, tf.tile, tf.matmul, tf.norm = reshape, split, concat, constant, tile, matmul, norm
    tf.square = lambda x: T(_raw(x) ** 2)
    tf.sqrt = lambda x: T(torch.sqrt(_raw(x)))
    tf.sigmoid = lambda x: T(torch.sigmoid(_raw(x)))
    tf.maximum = lambda a, b: T(torch.maximum(torch.as_tensor(_raw(a), dtype=DT), torch.as_tensor(_raw(b), dtype=DT)))
    tf.cast = lambda x, dtype=None: T(_raw(x).to(DT))
    tf.reduce_mean = _reduce(torch.mean)
    tf.reduce_sum = _reduce(torch.sum)
    tf.nn = types.SimpleNamespace(softmax=softmax, depthwise_conv2d=depthwise_conv2d,
                                  softmax_cross_entropy_with_logits=softmax_cross_entropy_with_logits)
    v1 = types.SimpleNamespace(variable_scope=variable_scope, losses=types.SimpleNamespace(add_loss=lambda loss: None))
    tf.compat = types.SimpleNamespace(v1=v1)
    mods = {"tensorflow": tf}
    for name in ("tensorflow.python", "tensorflow.python.ops", "tensorflow.python.ops.gen_nn_ops"):
        mods[name] = types.ModuleType(name)
    mods["tensorflow.python.ops.gen_nn_ops"].leaky_relu = leaky_relu
    slim = types.ModuleType("tf_slim")
    slim.conv2d, slim.fully_connected, slim.arg_scope, slim.batch_norm = conv2d, fully_connected, arg_scope, batch_norm
    mods["tf_slim"] = slim

    class ModelOutputTensors:
        def __init__(self, y_conv, image_output, image_original, histogram_tensors):
            self.y_conv, self.image_output, self.image_original = y_conv, image_output, image_original
            self.histogram_tensors = histogram_tensors

    class ModelInputParams:
        def __init__(self, x, y, device_id, is_training):
            self.x, self.y, self.device_id, self.is_training = x, y, device_id, is_training

    common = types.ModuleType("common")
    common.__path__ = []
    ops = types.ModuleType("common.common_nn_ops")  # (the reference's own imports the whole TensorFlow stack)
    ops.ModelOutputTensors, ops.ModelInputParams = ModelOutputTensors, ModelInputParams
    mods["common"], mods["common.common_nn_ops"] = common, ops
    sys.modules.update(mods)
    return list(mods)
