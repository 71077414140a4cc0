"""TEST INFRASTRUCTURE shared by tests/test_gpu_capsule_kernels.py (the HIP kernels of csrc/capsule.hip) and
tests/test_capsule_cases_emu.py (the emulation twins of tests/emu_capsule.py): named cases -- buffers, a call list, the
outputs to compare -- and a float64 reference that shares no backward algebra with either.

The reference writes only the FORWARD expressions in float64 torch (u_hat = x W + B, s = sum_i c u_hat, the squash with
its mean and eps, y = |v|, c = softmax(b), the label mask) and takes every backward result from torch.autograd.grad with
the kernel's cotangents.  The one place where it follows the kernel's documented convention instead: at a capsule whose
s is exactly zero, d|v| is NaN in autograd; include/hypel.h drops the gy term there, and so does `ref_head_bwd`.

Every output lies inside a larger allocation filled with a canary (parity_util.SENT); whatever lies outside the contract's
extent -- the guards, the pad columns of a strided dx, what follows n*i*jd, n*jd, n*j or i*j -- must keep its bits.

The fp32 yardstick of the edge cases (`F32R`): a plain float32 NumPy rendition of the same closed forms the kernels use,
float32 throughout except where the contract says float64 (the agreement sums, the logits, the softmax)."""
import math

import numpy as np
import torch

from hypelcnn_amd.backend import Ref
from tests.parity_util import SENT

F32 = np.float32
EPS = 1e-9
GUARD = 64  # canary elements before and after every output
KERNEL_TOL = 2e-5  # tests/test_gpu_capsule.py: one kernel, fp32 sums of at most a few thousand terms, of the largest entry
MARGIN = 4.0  # an edge-case tensor may be this many times as far from float64 as the fp32 rendition is (summation order)

# (n, pixels, m, j, d, terms); I = pixels * m.  Every I of {1, 7, 8, 9, 31, 32, 33, 64} (the 8 route waves, the unrolled
# loop's entry at i + 24 < I) and every n of {1, 3, 4, 5, 15, 16, 17, 33} (the 4 agree waves, the 16-sample tile) meets a
# width above 256 columns: 272 (a partly filled second slot), 320, 496 (the widest the backward admits at D = 16),
# 320 at D = 32 (one capsule per route group, full register arrays), 511 (D = 7).  Then J = 64 / D = 1 and J = 9 / D = 7
# (cw = 63: a group that ends mid-wave).
SHAPES = [(1, 1, 1, 17, 16, 1), (3, 7, 1, 20, 16, 3), (4, 4, 2, 31, 16, 5), (5, 3, 3, 10, 32, 5), (15, 31, 1, 73, 7, 3),
          (16, 8, 4, 17, 16, 5), (17, 11, 3, 20, 16, 3), (33, 16, 4, 31, 16, 5), (5, 2, 5, 64, 1, 3), (19, 5, 2, 9, 7, 5)]


def shape_id(s):
    return "n{}-I{}x{}-J{}-D{}-T{}".format(*s)


# ================================================================================================ float64 reference
def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def x_index(pix, ld, m, n, i, d):
    """element offsets of x[n][i][:] (include/hypel.h: pix[i / m] + n * ld + (i % m) * d): [n, i, d]"""
    idx = np.empty((n, i, d), np.int64)
    for ii in range(i):
        for nn in range(n):
            idx[nn, ii] = int(pix[ii // m]) + nn * ld + (ii % m) * d + np.arange(d)
    return idx


def squash(s):
    q = (s * s).mean(-1, keepdim=True)
    return q * s / ((1 + q) * torch.sqrt(q + EPS))


def ref_uhat(x, w, b):
    return torch.einsum("nid,idc->nic", x, w) + b


def ref_route_fwd(uhat, coef):
    s = torch.einsum("ij,nijd->njd", t64(coef), t64(uhat))
    v = squash(s)
    return s.numpy(), v.numpy(), torch.sqrt((v * v).sum(-1)).numpy()


def ref_route_bwd(uhat, coef, s_in):
    dv = torch.einsum("ij,nijd->njd", t64(coef), t64(uhat))
    s = t64(s_in, True)
    return torch.autograd.grad(squash(s), s, dv)[0].numpy()


def ref_head_bwd(gy, gv, s_in):
    s = t64(s_in, True)
    v = squash(s)
    total = 0.0
    if gy is not None:
        sq = (v * v).sum(-1)
        live = sq.detach() > 0  # the kernel's convention at the zero capsule: no gradient through |v|
        total = total + (t64(gy)[live] * torch.sqrt(sq[live])).sum()
    if gv is not None:
        total = total + (t64(gv) * v).sum()
    return torch.autograd.grad(total, s)[0].numpy()


def exact_agreement(uhat, vec):
    """sum_n sum_e uhat[n,i,j,e] * vec[n,j,e], correctly rounded: a product of two float32 is exact in float64 and
    math.fsum adds without error -- the float64 reference of the logit cases carries no summation noise of its own"""
    n, i, j, d = uhat.shape
    p = (uhat.astype(np.float64) * vec.astype(np.float64)[:, None]).transpose(1, 2, 0, 3).reshape(i, j, n * d)
    return np.array([[math.fsum(p[a, b]) for b in range(j)] for a in range(i)])


def ref_agree_fwd(uhat, vec, b_in, exact=False):
    a = t64(exact_agreement(uhat, vec)) if exact else torch.einsum("nijd,njd->ij", t64(uhat), t64(vec))
    b = a if b_in is None else a + t64(b_in)
    return b.numpy(), torch.softmax(b, 1).numpy()


def ref_agree_bwd(uhat, ds, b64, db_next, exact=False):
    """the VJP of the softmax AT THE FLOAT64 LOGITS (the kernel is handed their float32 coefficients), plus db_next"""
    dc = t64(exact_agreement(uhat, ds)) if exact else torch.einsum("nijd,njd->ij", t64(uhat), t64(ds))
    b = t64(b64, True)
    db = torch.autograd.grad(torch.softmax(b, 1), b, dc)[0]
    return (db if db_next is None else db + t64(db_next)).numpy()


def ref_uhat_bwd(xg, w, coefs, vecs):
    """gradients of sum(du * u_hat) with respect to W, B, x[n,i,d]; du = sum_t coefs[t] (x) vecs[t]"""
    t, i, j = coefs.shape
    n = vecs.shape[1]
    d = w.shape[1]
    X, W = t64(xg, True), t64(w, True)
    B = torch.zeros(i, j * d, dtype=torch.float64, requires_grad=True)
    du = torch.einsum("tij,tnjd->nijd", t64(coefs), t64(vecs).reshape(t, n, j, d)).reshape(n, i, j * d)
    gw, gb, gx = torch.autograd.grad((du * ref_uhat(X, W, B)).sum(), [W, B, X])
    return gw.numpy(), gb.numpy(), gx.numpy()


def ref_mask_fwd(v, labels):
    return torch.einsum("nj,njd->nd", t64(labels), t64(v)).numpy()


def ref_mask_bwd(v_shape, labels, gout):
    v = torch.zeros(v_shape, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(torch.einsum("nj,njd->nd", t64(labels), v), v, t64(gout))[0].numpy()


# ================================================================================================ fp32 rendition
class F32R:
    """float32 NumPy rendition of the kernels' closed forms: the yardstick of the edge cases"""

    @staticmethod
    def gain(q):
        return q / ((F32(1) + q) * np.sqrt(q + F32(EPS)))

    @staticmethod
    def gain_grad(q):
        qe = q + F32(EPS)
        return (qe - F32(0.5) * q * (F32(1) + q)) / ((F32(1) + q) * (F32(1) + q) * qe * np.sqrt(qe))

    @classmethod
    def squash_bwd(cls, s, dv):
        d = F32(s.shape[-1])
        q = (s * s).sum(-1, keepdims=True) / d
        dot = (s * dv).sum(-1, keepdims=True)
        return cls.gain(q) * dv + cls.gain_grad(q) * (F32(2) / d) * dot * s

    @staticmethod
    def route_sum(uhat, coef):
        acc = np.zeros(uhat.shape[:1] + uhat.shape[2:], F32)
        for i in range(uhat.shape[1]):
            acc += coef[i][None, :, None] * uhat[:, i]
        return acc

    @classmethod
    def route_fwd(cls, uhat, coef):
        s = cls.route_sum(uhat, coef)
        v = cls.gain((s * s).sum(-1, keepdims=True) / F32(s.shape[-1])) * s
        return s, v, np.sqrt((v * v).sum(-1))

    @classmethod
    def route_bwd(cls, uhat, coef, s_in):
        return cls.squash_bwd(s_in, cls.route_sum(uhat, coef))

    @classmethod
    def head_bwd(cls, gy, gv, s):
        v = cls.gain((s * s).sum(-1, keepdims=True) / F32(s.shape[-1])) * s
        nv = np.sqrt((v * v).sum(-1, keepdims=True))
        dv = np.zeros_like(s)
        if gy is not None:
            dv = dv + np.where(nv > 0, gy[..., None] / np.where(nv > 0, nv, F32(1)), F32(0)) * v
        if gv is not None:
            dv = dv + gv
        return cls.squash_bwd(s, dv)

    # the agreement kernels: float64 sums, logits and softmax by contract; float32 only in what they read and write
    @staticmethod
    def agree_sum(uhat, vec, dtype=np.float64):
        acc = np.zeros(uhat.shape[1:3], dtype)
        for n in range(uhat.shape[0]):
            for e in range(uhat.shape[3]):
                acc += uhat[n, :, :, e].astype(dtype) * vec[n, :, e].astype(dtype)[None]
        return acc

    @classmethod
    def agree_fwd(cls, uhat, vec, b_in, dtype=np.float64):
        b = cls.agree_sum(uhat, vec, dtype)
        if b_in is not None:
            b = b + b_in.astype(dtype)
        e = np.exp(b - b.max(1, keepdims=True))
        return b, (e / e.sum(1, keepdims=True)).astype(F32)

    @classmethod
    def agree_bwd(cls, uhat, ds, c, db_next, dtype=np.float64, cancelling=False):
        dc = cls.agree_sum(uhat, ds, dtype)
        c = c.astype(dtype)
        if cancelling:  # c_j (dc_j - <c, dc>): what the kernel's form avoids
            out = c * (dc - (c * dc).sum(1, keepdims=True))
        else:
            out = c * (c[:, None, :] * (dc[:, :, None] - dc[:, None, :])).sum(-1)
        if db_next is not None:
            out = out + db_next.astype(dtype)
        return out.astype(F32)


# ================================================================================================ error measures
def tensor_err(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-6))


def vector_err(got, ref, width):
    """Largest error of a capsule vector (a row of `width` entries) relative to THAT vector's largest reference entry: a
    wrong small capsule does not hide behind a large one.  A vector whose reference is all zero must be all zero (and
    finite) in `got`; returns (error over the other vectors, that condition)."""
    g = np.asarray(got, np.float64).reshape(-1, width)
    r = np.asarray(ref, np.float64).reshape(-1, width)
    scale = np.abs(r).max(1)
    zero = scale == 0
    zeros_ok = bool((g[zero] == 0).all())
    if zero.all():
        return 0.0, zeros_ok
    with np.errstate(invalid="ignore"):
        err = np.abs(g - r).max(1)[~zero] / scale[~zero]
    return float(np.nan_to_num(err, nan=np.inf).max()), zeros_ok


# ================================================================================================ cases
class Check:
    def __init__(self, label, buf, index, ref, width=0, key=None):
        """`buf`[`index`] (flat element numbers, any shape) against `ref` (float64, same shape).  width 0: the shape
        cases' measure (KERNEL_TOL of the tensor's largest entry); width > 0: per vector of that width, limit key `key`."""
        self.label, self.buf, self.index, self.ref, self.width, self.key = label, buf, np.asarray(index), ref, width, key


class Case:
    """Buffers (name -> initial flat array), a call list [(entry, args)] whose pointer arguments are buffer names or
    (name, element offset), and the checks.  Every output has a buffer of its own, so the checks run after all calls."""

    def __init__(self, name):
        self.name, self.bufs, self.calls, self.checks, self.outputs = name, {}, [], [], {}
        self.f32 = {}  # check label -> the fp32 rendition's result (edge cases)

    def inp(self, name, array, dtype=F32):
        self.bufs[name] = np.ascontiguousarray(array, dtype).reshape(-1).copy()
        return name

    def out(self, name, size, init=None, dtype=F32, tail=0):
        """A canary-filled allocation with `size` elements of extent behind GUARD elements; `init`: the extent's content
        (an accumulating call).  -> the pointer argument."""
        a = np.full(GUARD + size + tail + GUARD, SENT, dtype)
        if init is not None:
            a[GUARD:GUARD + size] = np.asarray(init, dtype).reshape(-1)
        self.bufs[name] = a
        self.outputs[name] = None
        return (name, GUARD)

    def call(self, entry, *args):
        self.calls.append((entry, args))

    def check(self, label, ptr, ref, width=0, key=None, index=None):
        name, off = ptr
        ref = np.asarray(ref, np.float64)
        index = off + np.arange(ref.size).reshape(ref.shape) if index is None else index
        self.checks.append(Check(label, name, index, ref, width, key))

    # ------------------------------------------------------------------------------------------------ running
    def run(self, backend):
        """-> {output buffer name: numpy array after all calls}"""
        store = {k: backend.upload(v) for k, v in self.bufs.items()}
        for entry, args in self.calls:
            backend.call(entry, *[Ref(store[a]) if isinstance(a, str) else Ref(store[a[0]], a[1]) if isinstance(a, tuple)
                                  else a for a in args])
        backend.synchronize()
        return {k: store[k].cpu().numpy() for k in self.outputs}

    def errors(self, res):
        """Asserts the canaries and the exact zeros; -> {check label: (error, width, key)}"""
        touched = {k: np.zeros(v.size, bool) for k, v in res.items()}
        out = {}
        for c in self.checks:
            got = res[c.buf][c.index]
            touched[c.buf][c.index.reshape(-1)] = True
            assert np.isfinite(got).all(), (self.name, c.label, "not finite")
            if c.width:
                err, zeros_ok = vector_err(got, c.ref, c.width)
                assert zeros_ok, (self.name, c.label, "a vector that is exactly zero in float64 is not exactly zero")
            else:
                err = tensor_err(got, c.ref)
            out[c.label] = (err, c.width, c.key)
        for k, v in res.items():
            keep = ~touched[k]
            same = v[keep].view(np.uint8).reshape(-1, v.itemsize) == self.bufs[k][keep].view(np.uint8).reshape(-1, v.itemsize)
            bad = np.flatnonzero(~same.all(1))
            assert bad.size == 0, (f"{self.name}: {bad.size} elements of `{k}` outside the contract's extent were written; "
                                   f"first at element {int(np.flatnonzero(keep)[bad[0]]) - GUARD} behind the guard")
        return out

    def f32_errors(self):
        """the fp32 rendition's error per edge check, by the same measure"""
        out = {}
        for c in self.checks:
            if c.label in self.f32:
                out[c.label] = vector_err(self.f32[c.label], c.ref, c.width)[0]
        return out


def assert_same_bits(a, b):
    """two runs of a case on identical inputs: every output buffer bit for bit"""
    for k in a:
        ta, tb = torch.from_numpy(a[k].view(np.uint8)), torch.from_numpy(b[k].view(np.uint8))
        assert torch.equal(ta, tb), f"`{k}` differs between two runs on identical inputs"


def _softmax64(b):
    e = np.exp(b - b.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


# ------------------------------------------------------------------------------------------------ shape cases
def shape_case(n, pixels, m, j, d, terms):
    """Every entry point in every call form the planner uses, on Gaussian inputs, each output against the float64
    reference of ITS inputs (the kernels do not feed each other: an input that is another kernel's output is the
    reference's, rounded to float32).  Views: x is a channel-offset window (column 2 of rows m*d + 3 wide) of a
    pixel-major buffer with shuffled pixels; dx goes through ANOTHER permutation, column 1 of rows m*d + 6 wide; the mask
    kernels get every leading dimension wider than its row."""
    rng = np.random.default_rng(1000 * n + 10 * j + d)
    c = Case(shape_id((n, pixels, m, j, d, terms)))
    i, jd = pixels * m, j * d
    ldx, lddx = m * d + 3, m * d + 6
    perm = rng.permutation(pixels).astype(np.int64)
    pix = perm * n * ldx + 2
    dpix = np.roll(perm, 1) * n * lddx + 1 + GUARD  # another order of the pixels whenever there are two
    r32 = lambda *shape, scale=1.0: (rng.standard_normal(shape) * scale).astype(F32)  # noqa: E731
    x, w, bias = r32(pixels * n * ldx), r32(i, d, jd, scale=0.5), r32(i, jd, scale=0.1)
    c.inp("x", x), c.inp("w", w), c.inp("bias", bias)
    c.inp("pix", pix, np.int64), c.inp("dpix", dpix, np.int64)
    xi = x_index(pix, ldx, m, n, i, d)
    xg = x[xi]
    uhat64 = ref_uhat(t64(xg), t64(w), t64(bias)).numpy()
    p = c.out("uhat", n * i * jd)
    c.call("caps_uhat_fwd", "x", "pix", ldx, m, "w", "bias", n, i, d, jd, p)
    c.check("uhat_fwd", p, uhat64)
    uhat = uhat64.astype(F32).reshape(n, i, j, d)
    c.inp("uhat_in", uhat)
    coef = rng.random((i, j)).astype(F32)
    coef /= coef.sum(1, keepdims=True)
    c.inp("coef", coef)
    s64, v64, y64 = ref_route_fwd(uhat, coef)
    for tag, with_y in (("", True), ("_noy", False)):
        ps, pv = c.out("s" + tag, n * jd), c.out("v" + tag, n * jd)
        py = c.out("y" + tag, n * j) if with_y else None
        c.call("caps_route_fwd", "uhat_in", "coef", n, i, j, d, ps, pv, py)
        c.check("route_fwd.s" + tag, ps, s64), c.check("route_fwd.v" + tag, pv, v64)
        if with_y:
            c.check("route_fwd.y", py, y64)
    s_in, v_in = s64.astype(F32), v64.astype(F32)
    c.inp("s_in", s_in), c.inp("v_in", v_in)
    b_in = rng.standard_normal((i, j)) * 0.3
    c.inp("b_in", b_in, np.float64)
    for tag, bi in (("", b_in), ("_nob", None)):
        pb, pc = c.out("b_out" + tag, i * j, dtype=np.float64), c.out("c_out" + tag, i * j)
        c.call("caps_agree_fwd", "uhat_in", "v_in", n, i, j, d, None if bi is None else "b_in", pb, pc)
        b64, c64 = ref_agree_fwd(uhat, v_in, bi)
        c.check("agree_fwd.b" + tag, pb, b64), c.check("agree_fwd.c" + tag, pc, c64)
    gy, gv = r32(n, j), r32(n, j, d)
    c.inp("gy", gy), c.inp("gv", gv)
    for tag, a, b in (("", gy, gv), ("_gy", gy, None), ("_gv", None, gv)):
        pd = c.out("ds_head" + tag, n * jd)
        c.call("caps_head_bwd", None if a is None else "gy", None if b is None else "gv", "s_in", n, j, d, pd)
        c.check("head_bwd" + tag, pd, ref_head_bwd(a, b, s_in))
    ds, db_next = r32(n, j, d), r32(i, j, scale=0.2)
    blog = rng.standard_normal((i, j)) * 1.5  # float64 logits; the kernel reads their coefficients in float32
    c.inp("ds", ds), c.inp("db_next", db_next), c.inp("c_in", _softmax64(blog))
    for tag, nxt in (("", db_next), ("_nonext", None)):
        pd = c.out("db" + tag, i * j)
        c.call("caps_agree_bwd", "uhat_in", "ds", n, i, j, d, "c_in", None if nxt is None else "db_next", pd)
        c.check("agree_bwd" + tag, pd, ref_agree_bwd(uhat, ds, blog, nxt))
    dbc = r32(i, j, scale=0.3)
    c.inp("dbc", dbc)
    pd = c.out("ds_prev", n * jd)
    c.call("caps_route_bwd", "uhat_in", "dbc", n, i, j, d, "s_in", pd)
    c.check("route_bwd", pd, ref_route_bwd(uhat, dbc, s_in))
    coefs, vecs = r32(terms, i, j, scale=0.3), r32(terms, n, jd)
    c.inp("coefs", coefs), c.inp("vecs", vecs)
    gw64, gb64, gx64 = ref_uhat_bwd(xg, w, coefs, vecs)
    dxi = x_index(dpix, lddx, m, n, i, d)
    dx_elems = pixels * n * lddx

    def dx_buffer(name, init):
        a = np.full(GUARD + dx_elems + GUARD, SENT, F32)
        if init is not None:
            a[dxi] = init
        c.bufs[name] = a
        c.outputs[name] = None
        return (name, 0)  # the guard is inside dpix

    w0, b0, x0 = r32(i, d, jd), r32(i, jd), r32(n, i, d)
    for tag, acc in (("", 0), ("_acc", 1)):
        pw, pb = c.out("dw" + tag, i * d * jd, w0 if acc else None), c.out("dbias" + tag, i * jd, b0 if acc else None)
        px = dx_buffer("dx" + tag, x0 if acc else None)
        c.call("caps_uhat_bwd", "x", "pix", ldx, m, "w", n, i, j, d, terms, "coefs", "vecs", pw, pb, acc, px, "dpix", lddx, acc)
        c.check("uhat_bwd.dw" + tag, pw, gw64 + (w0 if acc else 0)), c.check("uhat_bwd.dbias" + tag, pb, gb64 + (b0 if acc else 0))
        c.check("uhat_bwd.dx" + tag, px, gx64 + (x0 if acc else 0), index=dxi)
    px = dx_buffer("dx_only", None)  # frozen weights
    c.call("caps_uhat_bwd", "x", "pix", ldx, m, "w", n, i, j, d, terms, "coefs", "vecs", None, None, 0, px, "dpix", lddx, 0)
    c.check("uhat_bwd.dx_only", px, gx64, index=dxi)
    pw, pb = c.out("dw_only", i * d * jd), c.out("dbias_only", i * jd)  # the first layer: no gradient wanted for x
    c.call("caps_uhat_bwd", "x", "pix", ldx, m, "w", n, i, j, d, terms, "coefs", "vecs", pw, pb, 0, None, None, 0, 0)
    c.check("uhat_bwd.dw_only", pw, gw64), c.check("uhat_bwd.dbias_only", pb, gb64)
    # label mask: v, labels, out, gout and gv each in rows wider than their content
    ldv, ldl, ldo, ldg, ldgv = jd + 5, j + 3, d + 2, d + 1, jd + 7
    rows = lambda a, ld: np.pad(a.reshape(n, -1), ((0, 0), (0, ld - a.reshape(n, -1).shape[1])), constant_values=SENT)  # noqa: E731
    labels, gout, gv0 = r32(n, j), r32(n, d), r32(n, jd)
    c.inp("v_rows", rows(v_in, ldv)), c.inp("labels", rows(labels, ldl)), c.inp("gout", rows(gout, ldg))
    window = lambda ld, width: GUARD + np.arange(n)[:, None] * ld + np.arange(width)[None, :]  # noqa: E731
    pm = c.out("masked", n * ldo)
    c.call("caps_mask_fwd", "v_rows", ldv, "labels", ldl, n, j, d, pm, ldo)
    c.check("mask_fwd", pm, ref_mask_fwd(v_in, labels), index=window(ldo, d))
    gm64 = ref_mask_bwd((n, j, d), labels, gout).reshape(n, jd)
    for tag, acc in (("", 0), ("_acc", 1)):
        c.bufs["gv_rows" + tag] = np.full(GUARD + n * ldgv + GUARD, SENT, F32)
        c.outputs["gv_rows" + tag] = None
        if acc:
            c.bufs["gv_rows" + tag][window(ldgv, jd)] = gv0
        c.call("caps_mask_bwd", "gout", ldg, "labels", ldl, n, j, d, ("gv_rows" + tag, GUARD), ldgv, acc)
        c.check("mask_bwd" + tag, ("gv_rows" + tag, GUARD), gm64 + (gv0 if acc else 0), index=window(ldgv, jd))
    return c


# ------------------------------------------------------------------------------------------------ squash edges
# q = mean(s^2) of whole capsules: exactly zero; around eps = 1e-9; both sides of q = 1, where the gain's derivative
# changes sign; up to 1e8 (entries of 1e4, far beyond what a sum of coefficient-weighted predictions reaches).  Nothing
# is asserted beyond: the gain derivative's denominator (1 + q)^2 (q + eps)^1.5 overflows float32 at q ~ 1e11, its
# numerator q (1 + q) / 2 at q ~ 2e19.
SQUASH_Q = [0.0, 1e-14, 1e-10, 1e-9, 1e-8, 1e-4, 1.0 - 1e-3, 1.0 + 1e-3, 1e2, 1e8]


def squash_case():
    """n = 5, I = 9, J = 20 (each regime of SQUASH_Q twice), D = 16: u_hat is scaled per (sample, class) so that the
    float64 s of that capsule has exactly the wanted q; class 0 and 10 have u_hat = 0 (zero W and bias for a class).
    route_fwd, route_bwd and head_bwd (gy and gv, gy alone, gv alone), each measured per capsule vector."""
    rng = np.random.default_rng(20)
    n, i, j, d = 5, 9, 2 * len(SQUASH_Q), 16
    c = Case("squash")
    coef = rng.random((i, j)).astype(F32)
    coef /= coef.sum(1, keepdims=True)
    base = rng.standard_normal((n, i, j, d))
    s0 = np.einsum("ij,nijd->njd", coef.astype(np.float64), base)
    q = np.tile(np.asarray(SQUASH_Q), 2)
    uhat = (base * np.sqrt(q[None, :, None] / (s0 * s0).mean(-1, keepdims=True))[:, None]).astype(F32)
    assert not uhat[:, :, [0, len(SQUASH_Q)]].any()
    c.inp("uhat", uhat), c.inp("coef", coef)
    s64, v64, y64 = ref_route_fwd(uhat, coef)
    assert not s64[:, 0].any() and np.allclose((s64 * s64).mean(-1)[:, 1:len(SQUASH_Q)], q[1:len(SQUASH_Q)], rtol=1e-5)
    regimes = len(SQUASH_Q)

    def per_regime(tensor, ptr, ref, f32, width):
        """one check per (tensor, regime): the two classes of that q over all samples"""
        ref, f32 = np.asarray(ref).reshape(n, j, width), np.asarray(f32).reshape(n, j, width)
        for r in range(regimes):
            cls = np.asarray([r, r + regimes])
            index = ptr[1] + (np.arange(n)[:, None, None] * j + cls[None, :, None]) * width + np.arange(width)[None, None, :]
            label = f"{tensor}@q={SQUASH_Q[r]:g}"
            c.checks.append(Check(label, ptr[0], index, ref[:, cls], width, (tensor, r)))
            c.f32[label] = f32[:, cls]

    ps, pv, py = c.out("s", n * j * d), c.out("v", n * j * d), c.out("y", n * j)
    c.call("caps_route_fwd", "uhat", "coef", n, i, j, d, ps, pv, py)
    fs, fv, fy = F32R.route_fwd(uhat, coef)
    per_regime("route_fwd.s", ps, s64, fs, d), per_regime("route_fwd.v", pv, v64, fv, d), per_regime("route_fwd.y", py, y64, fy, 1)
    s_in = s64.astype(F32)
    c.inp("s_in", s_in)
    dbc = (rng.standard_normal((i, j)) * 0.3).astype(F32)
    c.inp("dbc", dbc)
    pd = c.out("ds_prev", n * j * d)
    c.call("caps_route_bwd", "uhat", "dbc", n, i, j, d, "s_in", pd)
    per_regime("route_bwd", pd, ref_route_bwd(uhat, dbc, s_in), F32R.route_bwd(uhat, dbc, s_in), d)
    gy, gv = rng.standard_normal((n, j)).astype(F32), rng.standard_normal((n, j, d)).astype(F32)
    c.inp("gy", gy), c.inp("gv", gv)
    for tag, a, b in (("", gy, gv), ("_gy", gy, None), ("_gv", None, gv)):
        pd = c.out("ds_head" + tag, n * j * d)
        c.call("caps_head_bwd", None if a is None else "gy", None if b is None else "gv", "s_in", n, j, d, pd)
        per_regime("head_bwd" + tag, pd, ref_head_bwd(a, b, s_in), F32R.head_bwd(a, b, s_in), d)
    return c


# ------------------------------------------------------------------------------------------------ routing logits
def logit_case():
    """n = 5, I = 12, J = 20, D = 16 (320 columns).  What the float64 sums, logits and softmax of the two agreement
    kernels are for; the float64 reference sums exactly (`exact_agreement`).

    agree_fwd: every class of a capsule shares one large agreement (b up to +-600 at n = 5) and differs by O(1), so the
      coefficients hang on differences a float32 b cannot hold (ulp(512) = 6e-5).  DEFEATS: float32 accumulation of the
      agreement, and float32 logits.  Rows 0-2 add b_in gaps of +800 / -800 / both (coefficients exactly 0 and 1: the
      float64 exp underflows), rows 3-4 have u_hat = 0 and equal b_in (exactly equal logits, c = 1/J).
    agree_bwd: dc rows of 1e4 + O(1) differences with c saturated (rows 0-2: exactly 0 and 1, db exactly 0 without
      db_next), uniform (rows 3-4) and spread (the rest).  DEFEATS: float32 accumulation of dc (ulp(1e4) = 1e-3), and
      the form c_j (dc_j - <c, dc>) on float32 coefficients, whose sum is 1 only to 1e-7 (an error of 1e-3 in <c, dc>)."""
    rng = np.random.default_rng(40)
    n, i, j, d = 5, 12, 20, 16
    c = Case("logits")

    def shared(target, spread):
        """(uhat [n,i,j,d], vec [n,j,d]) whose agreement is target[i] + O(spread) for every class"""
        vec = rng.standard_normal((n, 1, d)) * 0.22 + rng.standard_normal((n, j, d)) * 0.01
        common = vec.mean(1)
        u = target[None, :, None] * (common / (common * common).sum())[:, None, :]
        u = u[:, :, None, :] + rng.standard_normal((n, i, j, d)) * spread
        return u.astype(F32), vec.astype(F32)

    uhat, v = shared(np.linspace(-600.0, 600.0, i), 1.0)
    uhat[:, 3:5] = 0
    b_in = rng.standard_normal((i, j)) * 0.5
    b_in[0, 7] += 800.0
    b_in[1, 3] -= 800.0
    b_in[2, 5] += 800.0
    b_in[2, 6] -= 800.0
    b_in[3:5] = np.asarray([[3.5], [-117.25]])
    c.inp("uhat", uhat), c.inp("v", v), c.inp("b_in", b_in, np.float64)
    for tag, bi in (("", b_in), ("_nob", None)):
        pb, pc = c.out("b_out" + tag, i * j, dtype=np.float64), c.out("c_out" + tag, i * j)
        c.call("caps_agree_fwd", "uhat", "v", n, i, j, d, None if bi is None else "b_in", pb, pc)
        b64, c64 = ref_agree_fwd(uhat, v, bi, exact=True)
        c.check("agree_fwd.b" + tag, pb, b64, j, "agree_fwd.b" + tag), c.check("agree_fwd.c" + tag, pc, c64, j, "agree_fwd.c" + tag)
        c.f32["agree_fwd.b" + tag], c.f32["agree_fwd.c" + tag] = F32R.agree_fwd(uhat, v, bi)
        if bi is not None:
            assert np.abs(b64).max() > 300 and c64[0, 7] == 1.0 and c64[1, 3] == 0.0 and (c64[3:5] == c64[3, 0]).all()
    uhat2, ds = shared(np.full(i, 1e4), 1.0)
    blog = rng.standard_normal((i, j)) * 1.5
    blog[0, 7] += 800.0
    blog[1, 3] += 900.0
    blog[2, 0] += 2000.0
    blog[3:5] = np.asarray([[0.0], [41.5]])
    c_in = _softmax64(blog).astype(F32)
    assert c_in[0, 7] == 1.0 and c_in[0].sum() == 1.0 and (c_in[3:5] == F32(1.0 / j)).all()
    db_next = (rng.standard_normal((i, j)) * 0.2).astype(F32)
    c.inp("uhat2", uhat2), c.inp("ds", ds), c.inp("c_in", c_in), c.inp("db_next", db_next)
    for tag, nxt in (("", db_next), ("_nonext", None)):
        pd = c.out("db" + tag, i * j)
        c.call("caps_agree_bwd", "uhat2", "ds", n, i, j, d, "c_in", None if nxt is None else "db_next", pd)
        c.check("agree_bwd" + tag, pd, ref_agree_bwd(uhat2, ds, blog, nxt, exact=True), j, "agree_bwd" + tag)
        c.f32["agree_bwd" + tag] = F32R.agree_bwd(uhat2, ds, c_in, nxt)
    c.simplified = {  # what a float32 "simplification" of the kernels would return: must lie outside the limits
        "agree_fwd.c": F32R.agree_fwd(uhat, v, b_in, dtype=F32)[1],
        "agree_fwd.c_nob": F32R.agree_fwd(uhat, v, None, dtype=F32)[1],
        "agree_bwd_nonext": F32R.agree_bwd(uhat2, ds, c_in, None, dtype=F32),
        "agree_bwd_nonext/cancelling": F32R.agree_bwd(uhat2, ds, c_in, None, cancelling=True),
    }
    return c


_CACHE = {}


def get(name):
    """a case by name, built once per process (the reference is computed once and left unchanged)"""
    if name not in _CACHE:
        _CACHE[name] = squash_case() if name == "squash" else logit_case() if name == "logits" else shape_case(*name)
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------ refusals
# entry -> a valid small call (n = 2, i = 2, m = 1, j = 2, d = 2); "O" = a canary output, "I" = an input, "L" = int64 table
_N, _I, _M, _J, _D = 2, 2, 1, 2, 2
BASELINE = {
    "caps_uhat_fwd": dict(x="I", pix="L", ldx=4, m=_M, w="I", bias="I", n=_N, i=_I, d=_D, jd=_J * _D, uhat="O"),
    "caps_route_fwd": dict(uhat="I", coef="I", n=_N, i=_I, j=_J, d=_D, s="O", v="O", y="O"),
    "caps_route_bwd": dict(uhat="I", coef="I", n=_N, i=_I, j=_J, d=_D, s_in="I", ds_out="O"),
    "caps_agree_fwd": dict(uhat="I", v="I", n=_N, i=_I, j=_J, d=_D, b_in=None, b_out="O", c_out="O"),
    "caps_agree_bwd": dict(uhat="I", ds="I", n=_N, i=_I, j=_J, d=_D, c="I", db_next=None, db="O"),
    "caps_head_bwd": dict(gy="I", gv="I", s="I", n=_N, j=_J, d=_D, ds="O"),
    "caps_uhat_bwd": dict(x="I", pix="L", ldx=4, m=_M, w="I", n=_N, i=_I, j=_J, d=_D, n_terms=1, coefs="I", vecs="I", dw="O",
                          dbias="O", acc_w=0, dx="O", dpix="L", lddx=4, acc_x=0),
}
_SHAPED = list(BASELINE)
REFUSALS = ([(e, "d33", dict(d=33, jd=66) if e == "caps_uhat_fwd" else dict(d=33)) for e in _SHAPED]
            + [(e, "jd513", dict(d=27, jd=513) if e == "caps_uhat_fwd" else dict(j=19, d=27)) for e in _SHAPED]
            + [(e, "n0", dict(n=0)) for e in _SHAPED] + [(e, "n65536", dict(n=65536)) for e in _SHAPED]
            + [("caps_uhat_fwd", "i%m", dict(i=3, m=2)), ("caps_uhat_bwd", "i%m", dict(i=3, m=2)),
               ("caps_uhat_fwd", "jd%d", dict(jd=5)),
               ("caps_uhat_bwd", "dw_without_dbias", dict(dbias=None)), ("caps_uhat_bwd", "dbias_without_dw", dict(dw=None)),
               ("caps_uhat_bwd", "neither_dw_nor_dx", dict(dw=None, dbias=None, dx=None)),
               # the LDS overflows (include/hypel.h "Limits"; J = 32 / D = 16 / R = 3 asks for 67 328 bytes)
               ("caps_uhat_bwd", "lds_J32_D16_R3", dict(j=32, d=16, n_terms=5)),
               ("caps_uhat_bwd", "lds_J11_D32_R3", dict(j=11, d=32, n_terms=5)),
               ("caps_uhat_bwd", "lds_J16_D32_R3", dict(j=16, d=32, n_terms=5)),
               ("caps_uhat_fwd", "lds_J16_D32", dict(d=32, jd=512))])


def refusal_id(r):
    return f"{r[0]}-{r[1]}"


def refusal_args(entry, change):
    """-> (argument list with buffer names, {buffer name: array}); nothing is launched, so the buffers stay small"""
    spec = dict(BASELINE[entry], **change)
    args, bufs = [], {}
    for k, v in spec.items():
        if v in ("I", "O", "L"):
            bufs[k] = (np.zeros(64, np.int64) if v == "L" else np.full(256, SENT, np.float64 if k == "b_out" else F32)
                       if v == "O" else np.ones(256, F32))
            args.append(k)
        else:
            args.append(v)
    return args, bufs, [k for k, v in spec.items() if v == "O"]


# ------------------------------------------------------------------------------------------------ model level
# One training step of CAPModel through the planner above 256 prediction columns, everything else tiny: patch 3, 1 x 1
# kernels (9 pixels x 2 primary capsules = 18 capsules), batch 5, R = 3, decoder on.  (classes, width, seed); the seed is
# picked on the CPU with the emulation: qmin > 1e-6 and no ReLU pre-activation inside emu_capsule.KINK_ZONE
# (tests/test_capsule_cases_emu.py asserts both).  20 x 16 = 320 (GRSS2018); 31 x 16 = 496 and 10 x 32 = 320 are the
# widest shapes the backward admits at those widths.
MODEL_PATCH, MODEL_CHANNELS, MODEL_BATCH = 3, 5, 5
MODEL_CASES = [(20, 16, 1), (31, 16, 1), (10, 32, 1)]


def model_alg(width):
    return dict(iter_routing=3, conv_layer_kernel_size=1, primary_caps_kernel_size=1, feature_count=6,
                primary_capsule_count=2, digit_capsule_output_space=width, optimizer="AdamOptimizer", learning_rate=1e-4,
                learning_rate_decay_factor=0.96, learning_rate_decay_step=350, lrelu_alpha=0.18, enable_decoding=True)


def model_inputs(classes, width, seed):
    from tests import emu_capsule as EC
    alg = model_alg(width)
    rng = np.random.default_rng(seed)
    params = EC.init_params(MODEL_PATCH, MODEL_CHANNELS, classes, alg, rng, True)
    x = rng.random((MODEL_BATCH, MODEL_PATCH, MODEL_PATCH, MODEL_CHANNELS)).astype(F32)
    onehot = np.eye(classes, dtype=F32)[rng.integers(0, classes, MODEL_BATCH)]
    return alg, params, x, onehot
