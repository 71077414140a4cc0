"""TEST INFRASTRUCTURE shared by tests/test_gpu_gan_stacks.py, tests/test_gpu_gan_losses.py (the HIP kernels against the
float64 spec of tests/emu_backend.py) and tests/test_gan_kernel_cases_emu.py (the same cases through the spec alone): the
case tables, the operand layouts and the checks, which run unchanged on `Both` and on `SpecOnly` (tests/parity_util.py).

Every row operand of a strided case is a slice: its own leading dimension, its own column offset (odd ones included, so
the base is only 4-byte aligned), inside a sentinel-filled allocation (parity_util.Arena).  The planner calls the kernels
this way (hypelcnn_amd/plan_gan.py hands them `buffer + ch_off, ld`)."""
import numpy as np

from hypelcnn_amd.backend import LOSS_NONE, LOSS_TERM_DTYPE
from tests import emu_backend
from tests.emu_backend import generator_knife_edge_rows
from tests.parity_util import SENT, Arena, assert_close, assert_same_bits, bits

F32 = np.float32
ULP = float(np.finfo(np.float32).eps)  # both sides round their result to float32: they may differ by one ulp of it


def _seed(*parts):
    h = 17
    for p in parts:
        for ch in str(p):
            h = (h * 131 + ord(ch)) % (1 << 31)
    return h


def fetch(b, name):
    """(device, spec) host copies of a named array"""
    return b.h[name].cpu().numpy().copy(), b.e[name].cpu().numpy().copy()


# ================================================================================================== fused generator
# tolerances of the existing test of the same entry point (tests/test_gpu_kernels.py): (rtol, atol * max(1, max|ref|))
GEN_TOL = {
    "plain": dict(out=(5e-5, 5e-6), dx=(1e-4, 1e-5), dw=(2e-4, 2e-5), db=(2e-4, 2e-5)),
    "keep": dict(out=(5e-5, 5e-6), dx=(1e-4, 1e-5), dw=(2e-4, 2e-5), db=(2e-4, 2e-5)),  # bit-identical to "plain"
    "tap": dict(out=(2e-4, 2e-5), enc=(2e-4, 2e-5), dx=(5e-4, 5e-5), dw=(5e-4, 5e-5), db=(5e-4, 5e-5)),
    "apps": dict(out=(2e-4, 2e-5), dx=(5e-4, 5e-5), dw=(5e-4, 5e-5), db=(5e-4, 5e-5)),
}
GEN_SCALE = {"plain": (0.3, 0.05), "keep": (0.3, 0.05), "tap": (0.4, 0.1), "apps": (0.4, 0.1)}  # as those tests draw
MFMA_ONLY = ("keep", "tap", "apps")  # entry points of the matrix-core kernels (16 <= bands <= 368, HYPEL_GAN_MFMA != 0)

GEN_STRIDED_SHAPES = [(64, 1), (64, 17), (16, 5), (20, 19), (144, 37), (360, 33)]
GEN_STRIDED = [(entry, bands, n, enc) for entry in ("plain", "keep", "tap", "apps") for bands, n in GEN_STRIDED_SHAPES
               for enc in (0, 1) if not (entry == "tap" and enc)]
# more row tiles than blocks: forward 2 * blocks(n) = 1024 blocks of 16 rows, two of them walk two tiles, the last tile
# has 5 rows; backward 512 blocks, two walk two tiles, the last tile has 3 rows
GEN_WALK_FWD = (16, 16 * 1024 + 16 + 5)
GEN_WALK_BWD = (48, 8192 + 16 + 3)
# 8, 12: wave-per-sample; 17-31: a second column tile that is mostly padding; 368: the last matrix-core count (the LDS
# rule of hypel_gm_supported; the documents said 384 until these cases ran), 369 and 384: the register-tiled kernel in
# the default process; 386: above the tiling's 384 -- the largest count whose backward fits the LDS rule of
# gan_generator_bwd_impl is 388 (163 280 of 163 328 bytes; 386: 162 992), and 386 is what runs here
GEN_EDGE_BANDS = [8, 12, 16, 17, 24, 31, 368, 369, 384, 386]
GEN_MFMA_LAST = 368
GEN_EDGE_N = [9, 33]
GEN_ZERO = [("plain", 64, 0), ("plain", 64, 1), ("keep", 64, 0), ("keep", 360, 1), ("plain", 360, 0), ("plain", 12, 0),
            ("plain", 12, 1), ("keep", 16, 0)]
GEN_ZERO_N = 18
GEN_NAN = [("plain", 64), ("keep", 64), ("plain", 360), ("keep", 360), ("plain", 12)]
NAN_N, NAN_ROW = 35, 17  # the poisoned row shares the tile of rows 16..31; the last tile has 3 rows


def case_id(case):
    """ids of the parametrised tests; `mfma_only` marks what the HYPEL_GAN_MFMA=0 child process leaves out"""
    s = "-".join("x".join(str(v) for v in c) if isinstance(c, (tuple, list)) else str(c) for c in case)
    return s + "-mfma_only" if case[0] in MFMA_ONLY else s


def gen_ks(bands):
    return [bands >> s for s in (0, 1, 2, 3, 2, 1, 0)]


def gen_layout(bands):
    """operand -> (ld, column): pairwise different lds; at 64 bands x 3/73, out 1/70, dout 2/67, dx 5/81"""
    return {"x": (bands + 9, 3), "out": (bands + 6, 1), "dout": (bands + 3, 2), "dx": (bands + 17, 5),
            "enc": (bands + 12, 7), "denc": (bands + 14, 4)}


class GenCase:
    """One generator shape with its operands; run() launches forward + backward of one entry point in one layout."""

    def __init__(self, entry, bands, n, enc, zero_rows=False, seed_extra=""):
        self.entry, self.bands, self.n, self.enc = entry, bands, n, enc
        self.apps = 2 if entry == "apps" else 1
        rng = np.random.default_rng(_seed(entry, bands, n, enc, seed_extra))
        ks = gen_ks(bands)
        self.wt = wt = sum(ks)
        gap_w, gap_b = (40, 24) if self.apps > 1 else (0, 0)  # the second model's variables: a fixed distance behind
        self.w_stride, self.b_stride = wt + gap_w, 8 + gap_b
        wscale, bscale = GEN_SCALE[entry]
        self.w = np.zeros(self.apps * self.w_stride, F32)
        self.bias = np.zeros(self.apps * self.b_stride, F32)
        rows = self.apps * n
        self.x = rng.random((rows, bands)).astype(F32)
        # (branch convention at zero) every other row exactly zero and no biases: every pre-activation of those rows is
        # exactly 0 in fp32 and in float64
        self.fixed = np.arange(0, rows, 2) if zero_rows else np.zeros(0, int)
        self.x[self.fixed] = 0.0
        for g in range(self.apps):
            wg = (rng.standard_normal(wt) * wscale / np.sqrt(np.repeat(ks, ks))).astype(F32)
            bg = np.zeros(8, F32) if zero_rows else (rng.standard_normal(8) * bscale).astype(F32)
            self.w[g * self.w_stride: g * self.w_stride + wt] = wg
            self.bias[g * self.b_stride: g * self.b_stride + 8] = bg
            xs = self.x[g * n:(g + 1) * n]
            fixed = self.fixed[(self.fixed >= g * n) & (self.fixed < (g + 1) * n)] - g * n
            # samples whose leaky-ReLU branch hangs on the rounding of an fp32 sum are re-drawn, never dropped
            for _ in range(20):
                bad = np.setdiff1d(generator_knife_edge_rows(xs, wg, bg, bands, bool(enc)), fixed)
                if len(bad) == 0:
                    break
                xs[bad] = rng.random((len(bad), bands)).astype(F32)
            assert len(bad) == 0, "knife-edge rows left after 20 rounds"
            if zero_rows:
                assert len(generator_knife_edge_rows(xs, wg, bg, bands, bool(enc))) == len(fixed), "the zero rows sit ON the kink"
        self.dout = rng.standard_normal((rows, bands)).astype(F32)
        self.denc = rng.standard_normal((rows, bands)).astype(F32)
        self.dx0 = rng.standard_normal((rows, bands)).astype(F32)
        self.kept = entry == "keep" or (entry in ("tap", "apps") and bands in (64, 360, 20))

    def run(self, b, strided, acc=1, want_dx=True, x=None, bwd=True):
        """-> {name: (device array, spec array)}: out, enc, dx as [rows x bands] windows; pw, pb whole; dw, db summed"""
        q, B, n, A, enc, wt = b.hip, self.bands, self.n, self.apps, self.enc, self.wt
        rows = A * n
        lay = gen_layout(B)
        arenas = {}

        def put(name, data):
            if strided:
                a = arenas[name] = Arena(rows, B, lay[name][0], lay[name][1], data)
                b.arr(name, a.buf)
                return (name, a.off), a.ld
            b.arr(name, np.full((rows, B), SENT, F32) if data is None else data)
            return name, B

        def get(name):
            h, e = fetch(b, name)
            if strided:
                arenas[name].check(h, name)
                arenas[name].check(e, name + " (spec)")
                return arenas[name].window(h).copy(), arenas[name].window(e).copy()
            return h.reshape(rows, B), e.reshape(rows, B)

        X, ldx = put("x", self.x if x is None else x)
        OUT, ldo = put("out", None)
        b.arr("w", self.w)
        b.arr("bias", self.bias)
        keep = None
        if self.kept:
            kf = q.gan_generator_keep_floats(n, B, enc)
            assert kf > 0
            keep = b.arr("keep", np.zeros(A * max(16, kf), F32))
        e = self.entry
        if e in ("plain", "keep"):
            b.run("gan_generator_fwd_keep" if e == "keep" else "gan_generator_fwd", X, ldx, n, B, "w", "bias", enc, OUT, ldo,
                  *([keep] if e == "keep" else []))
        elif e == "tap":
            ENC, lde = put("enc", None)
            b.run("gan_generator_fwd_tap", X, ldx, n, B, "w", "bias", OUT, ldo, ENC, lde, keep)
        else:
            b.run("gan_generator_fwd_apps", X, ldx, n, A, self.w_stride, self.b_stride, B, "w", "bias", enc, OUT, ldo, keep)
        res = {"out": get("out")}
        if e == "tap":
            res["enc"] = get("enc")
        if not bwd:
            return res
        DOUT, lddo = put("dout", self.dout)
        DX, lddx = put("dx", self.dx0)
        if A == 1:
            blocks = bpa = q.gan_generator_blocks(n)
            assert blocks == b.emu.gan_generator_blocks(n)
            pws, pbs, tail = blocks * wt, blocks * 8, 64
        else:
            blocks = q.gan_generator_blocks_apps(n, A)
            assert blocks % A == 0 and blocks <= 512 and blocks == b.emu.gan_generator_blocks_apps(n, A)
            bpa = blocks // A
            pws, pbs, tail = bpa * wt + 3 * wt + 5, bpa * 8 + 16, 0  # own regions, other slabs in between
        b.arr("pw", np.full(A * pws + tail, SENT, F32))
        b.arr("pb", np.full(A * pbs + tail, SENT, F32))
        dxa = DX if want_dx else None
        if e in ("plain", "keep"):
            b.run("gan_generator_bwd_kept" if e == "keep" else "gan_generator_bwd", X, ldx, DOUT, lddo, n, B, "w", "bias", enc,
                  dxa, lddx, acc, "pw", "pb", *([keep] if e == "keep" else []))
        elif e == "tap":
            DENC, ldde = put("denc", self.denc)
            b.run("gan_generator_bwd_tap", X, ldx, DOUT, lddo, DENC, ldde, n, B, "w", "bias", dxa, lddx, acc, "pw", "pb", keep)
        else:
            b.run("gan_generator_bwd_apps", X, ldx, DOUT, lddo, n, A, self.w_stride, self.b_stride, pws, pbs, B, "w", "bias",
                  enc, dxa, lddx, acc, "pw", "pb", keep)
        res["dx"] = get("dx")
        res["pw"], res["pb"] = fetch(b, "pw"), fetch(b, "pb")
        for nm, per, stride, used in (("pw", wt, pws, bpa * wt), ("pb", 8, pbs, bpa * 8)):  # nothing outside the slabs
            for arr in res[nm]:
                flat = arr[:A * stride].reshape(A, stride)[:, used:]
                assert (bits(flat) == bits(SENT)).all() and (bits(arr[A * stride:]) == bits(SENT)).all(), nm + ": beyond the slabs"
        b.arr("dw", np.zeros(A * wt, F32))
        b.arr("db", np.zeros(A * 8, F32))
        for g in range(A):
            b.run("reduce_splits_f32", ("pw", g * pws), wt, bpa, ("dw", g * wt), wt, 0, None, 0, 0)
            b.run("reduce_splits_f32", ("pb", g * pbs), 8, bpa, ("db", g * 8), 7, 0, None, 0, 0)
        res["dw"], res["db"] = fetch(b, "dw"), fetch(b, "db")
        return res

    def parity(self, res, names=None, tol=None):
        for nm in names or [k for k in res if k not in ("pw", "pb")]:
            rtol, atol = (tol or {}).get(nm) or GEN_TOL[self.entry][nm]
            assert_close(f"{self.entry} B={self.bands} n={self.n} {nm}", res[nm][0], res[nm][1], rtol, atol)


def assert_finite(res):
    for nm, (h, e) in res.items():
        assert np.isfinite(h).all() and np.isfinite(e).all(), nm


def check_strided(case, b):
    """(a) spec parity, (b) bit identity with the contiguous launch, (c) sentinels (inside run), (d) both accumulate
    flags on a pre-filled dx, (e) dx = NULL leaves the slabs as they are with dx given.  For GenCase and DenseCase."""
    s = case.run(b, True)
    c = case.run(b, False)
    case.parity(s)
    assert_finite(s)
    for nm in s:  # ld only enters addresses: no kernel has a reason to differ
        assert_same_bits(nm, s[nm][0], c[nm][0])
        assert_same_bits(nm + " (spec)", s[nm][1], c[nm][1])
    s0 = case.run(b, True, acc=0)
    case.parity(s0, ["dx"])
    assert not np.array_equal(s0["dx"][1], s["dx"][1]), "the two accumulate flags give different dx"
    sn = case.run(b, True, want_dx=False)
    for nm in ("pw", "pb"):
        assert_same_bits(nm + " without dx", sn[nm][0], s[nm][0])
    assert_same_bits("dx untouched", sn["dx"][0], case.dx0)


def check_zero_rows(case, b):
    """The `> 0` convention of the leaky-ReLU branch: a pre-activation of exactly 0 takes slope 0.1."""
    r = case.run(b, False)
    case.parity(r)
    z = case.fixed
    for nm in ("out", "dx"):
        tol = GEN_TOL[case.entry][nm]
        assert_close(nm + " of the zero rows", r[nm][0][z], r[nm][1][z], *tol)
    if not case.enc:
        assert (r["out"][0][z] == 0).all()
    return r


def check_row_independence(case, b):
    """One row of x is NaN: every other row of out and dx keeps its bits (dw / db are sums over all rows: not compared)."""
    clean = case.run(b, False)
    x = case.x.copy()
    x[NAN_ROW] = np.nan
    with np.errstate(all="ignore"):
        dirty = case.run(b, False, x=x)
    others = np.arange(case.x.shape[0]) != NAN_ROW
    for nm in ("out", "dx"):
        assert_same_bits(nm + " of the other rows", dirty[nm][0][others], clean[nm][0][others])
        assert np.isfinite(clean[nm][0]).all()
    assert np.isnan(dirty["out"][0][NAN_ROW]).all(), "the poisoned row is NaN"


# ===================================================================================================== dense stack
DENSE_TOL = {1: dict(out=(2e-5, 2e-6), dx=(5e-5, 5e-6), dw=(1e-4, 1e-5), db=(1e-4, 1e-5)),   # test_dense_stack_fwd_bwd
             2: dict(out=(2e-4, 2e-5), dx=(5e-4, 5e-5), dw=(5e-4, 5e-5), db=(5e-4, 5e-5))}  # ..._two_variable_sets_...
DENSE_STRIDED = [(widths, n, apps, sl) for apps in (1, 2) for n in (1, 17, 50) for widths, sl in
                 [((9, 64, 2), 0), ((9, 64, 2), 3), ((9, 64, 2), 6), ((64, 64, 64, 32), None), ((17, 5), None),
                  ((128, 128, 1), None), ((128, 24, 1), None), ((2, 128, 2), None)]]
# (128, 128, 1) does not fit: at a widest layer of 128 the LDS pitch is 146 floats, the two weight images alone take
# 2 * 128 * 146 * 4 = 149.5 KB of the 160 KB and the row images 18 KB (forward) / 73 KB (backward);
# hypel_dense_stack_supported says so and the planner then runs the layers as GEMMs.  The case stays in the table: the
# device test holds the library to refusing it -- an error, nothing launched -- on all its entry points.  (128, 24, 1)
# is the widest stack of that kind that runs (sum of the input widths rounded up to 4 <= 152).
DENSE_UNSUPPORTED = [(128, 128, 1)]
# several tiles per block (n > 4096; n > 2048 per application) with an input narrower than the hidden layers and a
# ragged last tile after a full one: LDS-weight path; register-weight forward (9856 weights >= 8192, widths <= 64); 128
DENSE_WALK = [((10, 64, 64, 2), 1), ((24, 64, 64, 64, 2), 1), ((9, 128, 5), 1), ((10, 64, 64, 2), 2),
              ((24, 64, 64, 64, 2), 2), ((9, 128, 5), 2)]
DENSE_WALK_N = {1: 4096 + 16 + 3, 2: 2048 + 16 + 3}
DENSE_EDGE = [(1, 128, 1), (128, 1, 128), (128, 16, 128)]
DENSE_NAN = (64, 64, 64, 32)


def dense_knife_edge_rows(x, ws, bs, lrelu, alpha, eps=1e-6):
    a = np.asarray(x, np.float64)
    near = np.zeros(len(a), bool)
    for wl, bl, act in zip(ws, bs, lrelu):
        v = a @ wl.astype(np.float64) + bl
        if act:
            near |= (np.abs(v) < eps).any(axis=1)
        a = np.where(v > 0, v, alpha * v) if act else v
    return np.nonzero(near)[0]


class DenseCase:
    def __init__(self, widths, n, apps=1, slice_i=None):
        self.widths, self.n, self.apps, self.entry = list(widths), n, apps, ("apps" if apps > 1 else "single")
        rng = np.random.default_rng(_seed("dense", widths, n, apps, slice_i))
        W = self.widths
        self.L = L = len(W) - 1
        self.act_mask, self.alpha = (1 << min(2, L - 1)) - 1, 0.1
        self.wt, self.bt = sum(a * c for a, c in zip(W, W[1:])), sum(W[1:])
        gap_w, gap_b = (52, 12) if apps > 1 else (0, 0)
        self.w_stride, self.b_stride = self.wt + gap_w, self.bt + gap_b
        self.w = np.zeros(apps * self.w_stride, F32)
        self.bias = np.zeros(apps * self.b_stride, F32)
        rows = apps * n
        self.x = rng.standard_normal((rows, W[0])).astype(F32)
        lrelu = [bool((self.act_mask >> l) & 1) for l in range(L)]
        for g in range(apps):
            ws = [(rng.standard_normal((a, c)) * np.sqrt(2.0 / a)).astype(F32) for a, c in zip(W, W[1:])]
            bs = [(rng.standard_normal(c) * 0.1).astype(F32) for c in W[1:]]
            self.w[g * self.w_stride: g * self.w_stride + self.wt] = np.concatenate([m.reshape(-1) for m in ws])
            self.bias[g * self.b_stride: g * self.b_stride + self.bt] = np.concatenate(bs)
            xs = self.x[g * n:(g + 1) * n]
            for _ in range(20):  # as for the generator: a branch decided by fp32 rounding is not a parity question
                bad = dense_knife_edge_rows(xs, ws, bs, lrelu, self.alpha)
                if len(bad) == 0:
                    break
                xs[bad] = rng.standard_normal((len(bad), W[0])).astype(F32)
            assert len(bad) == 0, "knife-edge rows left after 20 rounds"
        self.dout = rng.standard_normal((rows, W[-1])).astype(F32)
        self.dx0 = rng.standard_normal((rows, W[0])).astype(F32)
        c0, cl = W[0], W[-1]
        if slice_i is None:
            self.lay = {"x": (c0 + 9, 3), "out": (cl + 6, 1), "dout": (cl + 3, 2), "dx": (c0 + 17, 5)}
        else:  # slice i of an [n x 64] encoder output into slice i of an [n x 14] stack (the CUT feature stacks)
            i = slice_i
            self.lay = {"x": (64, c0 * i), "out": (14, cl * i), "dout": (17, cl * i + 1), "dx": (81, c0 * i + 5)}
        assert len({ld for ld, _ in self.lay.values()}) == 4

    def run(self, b, strided, acc=1, want_dx=True, x=None, bwd=True, fwd=True):
        q, n, A, W, L, wt, bt = b.hip, self.n, self.apps, self.widths, self.L, self.wt, self.bt
        rows = A * n
        width = {"x": W[0], "dx": W[0], "out": W[-1], "dout": W[-1]}
        arenas = {}

        def put(name, data):
            if strided:
                a = arenas[name] = Arena(rows, width[name], self.lay[name][0], self.lay[name][1], data)
                b.arr(name, a.buf)
                return (name, a.off), a.ld
            b.arr(name, np.full((rows, width[name]), SENT, F32) if data is None else data)
            return name, width[name]

        def get(name):
            h, e = fetch(b, name)
            if strided:
                arenas[name].check(h, name)
                arenas[name].check(e, name + " (spec)")
                return arenas[name].window(h).copy(), arenas[name].window(e).copy()
            return h.reshape(rows, width[name]), e.reshape(rows, width[name])

        shape = (L, *(W + [0] * (5 - len(W))), self.act_mask, self.alpha)
        X, ldx = put("x", self.x if x is None else x)
        OUT, ldo = put("out", None)
        b.arr("w", self.w)
        b.arr("bias", self.bias)
        if not fwd:
            pass
        elif A == 1:
            b.run("dense_stack_fwd", X, ldx, n, *shape, "w", "bias", OUT, ldo)
        else:
            b.run("dense_stack_fwd_apps", X, ldx, n, A, self.w_stride, self.b_stride, *shape, "w", "bias", OUT, ldo)
        res = {"out": get("out")}
        if not bwd:
            return res
        DOUT, lddo = put("dout", self.dout)
        DX, lddx = put("dx", self.dx0)
        if A == 1:
            bpa = q.dense_stack_blocks(n)
            assert bpa == b.emu.dense_stack_blocks(n)
            pws, pbs, tail = bpa * wt, bpa * bt, 64
        else:
            blocks = q.dense_stack_blocks_apps(n, A)
            assert blocks % A == 0 and blocks <= 256 and blocks == b.emu.dense_stack_blocks_apps(n, A)
            bpa = blocks // A
            pws, pbs, tail = bpa * wt + wt + 9, bpa * bt + 8, 0
        b.arr("pw", np.full(A * pws + tail, SENT, F32))
        b.arr("pb", np.full(A * pbs + tail, SENT, F32))
        dxa = DX if want_dx else None
        if A == 1:
            b.run("dense_stack_bwd", X, ldx, DOUT, lddo, n, *shape, "w", "bias", dxa, lddx, acc, "pw", "pb")
        else:
            b.run("dense_stack_bwd_apps", X, ldx, DOUT, lddo, n, A, self.w_stride, self.b_stride, pws, pbs, *shape, "w", "bias",
                  dxa, lddx, acc, "pw", "pb")
        res["dx"] = get("dx")
        res["pw"], res["pb"] = fetch(b, "pw"), fetch(b, "pb")
        for nm, stride, used in (("pw", pws, bpa * wt), ("pb", pbs, bpa * bt)):
            for arr in res[nm]:
                flat = arr[:A * stride].reshape(A, stride)[:, used:]
                assert (bits(flat) == bits(SENT)).all() and (bits(arr[A * stride:]) == bits(SENT)).all(), nm + ": beyond the slabs"
        b.arr("dw", np.zeros(A * wt, F32))
        b.arr("db", np.zeros(A * bt, F32))
        for g in range(A):
            b.run("reduce_splits_f32", ("pw", g * pws), wt, bpa, ("dw", g * wt), wt, 0, None, 0, 0)
            b.run("reduce_splits_f32", ("pb", g * pbs), bt, bpa, ("db", g * bt), bt, 0, None, 0, 0)
        res["dw"], res["db"] = fetch(b, "dw"), fetch(b, "db")
        return res

    def parity(self, res, names=None, tol=None):
        for nm in names or [k for k in res if k not in ("pw", "pb")]:
            rtol, atol = (tol or {}).get(nm) or DENSE_TOL[self.apps][nm]
            assert_close(f"dense {self.widths} n={self.n} apps={self.apps} {nm}", res[nm][0], res[nm][1], rtol, atol)


# ================================================================================== measured tolerances (new regimes)
def f32_error(launch, names, floor=1.0):
    """max |float32 evaluation - float64 spec| / max(floor, max|spec|) per named output: `launch(b)` runs on a SpecOnly
    and returns {name: (array, array)}.  The yardstick of operand regimes no older test compares with the spec (sums over
    more than 8000 samples or 300 000 weights, logits near 200, norms next to the clamp): 4 x this is allowed on the
    device -- the margin covers its other summation order and its expf / logf / tanhf."""
    from tests.parity_util import SpecOnly
    ref = launch(SpecOnly())
    with emu_backend.spec_dtype(np.float32):
        low = launch(SpecOnly())
    return {nm: float(np.abs(low[nm][0].astype(np.float64) - ref[nm][0]).max() / max(floor, np.abs(ref[nm][0]).max()))
            for nm in names}


# largest figures of f32_error seen over three draws of each of the two GEN_WALK_BWD cases (only_encoder 0 / 1):
# dw 8.3e-7, db 3.4e-6 of max(1, max|spec|); the device is allowed 4 x that (its sums run in another order)
GEN_WALK_F32_ERR = dict(dw=8.3e-7, db=3.4e-6)
MEASURED_FACTOR = 4.0


def measured_tol(err):
    """(rtol, atol) of a new regime: 4 x the float32 yardstick, and never below one ulp of the float32 result that both
    sides round to"""
    return 0.0, max(MEASURED_FACTOR * err, ULP)


def assert_close_rel(name, got, ref, err):
    """the same bound relative to max|ref| itself (no floor of 1): for outputs far from 1, as near the l2norm clamp"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    worst, allowed = np.abs(got - ref).max(), max(MEASURED_FACTOR * err, ULP) * np.abs(ref).max()
    assert worst <= allowed, f"{name}: max |got - spec| {worst:.3e} > {allowed:.3e}"


# ======================================================================================================= loss tail
class Ops:
    """The row operands of one loss launch, each an arena slice of its own; get() checks the sentinels on the way out."""

    def __init__(self, b):
        self.b, self.a = b, {}

    def put(self, name, data, rows, width, ld, col):
        a = self.a[name] = Arena(rows, width, ld, col, data)
        self.b.arr(name, a.buf)
        return (name, a.off), ld

    def get(self, name):
        h, e = fetch(self.b, name)
        self.a[name].check(h, name)
        self.a[name].check(e, name + " (spec)")
        return self.a[name].window(h).copy(), self.a[name].window(e).copy()


def close_all(res, tol, label=""):
    """tol: {name prefix: (rtol, atol)}; the longest matching prefix wins"""
    for nm, (h, e) in res.items():
        key = max((k for k in tol if nm.startswith(k)), key=len)
        assert_close(f"{label} {nm}", h, e, *tol[key])


# ---- patch-NCE: (6, 2), (7, 2) are the compile-time kernels, the rest runs the generic one
NCE_PE = [(6, 2), (7, 2), (5, 3), (1, 4), (8, 2)]
NCE_N = [1, 63, 65, 777]
NCE_TOL = {"loss": (1e-4, 1e-5), "dg": (2e-3, 1e-5), "dr": (2e-3, 1e-5)}  # test_gan_losses_l2norm_nce
# (dg given, acc_dg, dr given, acc_dr, accumulate_loss): dg only, dr only, neither, both flags on pre-filled gradients
NCE_STEPS = [(1, 0, 1, 1, 1), (1, 1, 1, 0, 1), (1, 1, 0, 0, 0), (0, 0, 1, 1, 1), (0, 0, 0, 0, 1), (1, 0, 0, 0, 0)]
NCE_BIG = [(7, 2), (5, 3)]  # |logit / tau| up to 200
NCE_BIG_N = 65
# f32_error of the two NCE_BIG cases (largest over loss / dg / dr and the steps): see run_nce
NCE_BIG_F32_ERR = {(7, 2): 2.04e-6, (5, 3): 1.0e-6}


def run_nce(b, p, e, n, big=False, zero_g=False, tau=0.07, weight=10.0):
    rng = np.random.default_rng(_seed("nce", p, e, n, big))
    pe = p * e
    g = (rng.standard_normal((n, pe)) * 0.3).astype(F32)
    r = (rng.standard_normal((n, pe)) * 0.3).astype(F32)
    if big:  # scaled so that the largest |logit / tau| is 200 (expf of -400 .. 0 after the max is taken out)
        top = np.abs(np.einsum("npe,nqe->npq", g.reshape(n, p, e).astype(np.float64), r.reshape(n, p, e))).max()
        g, r = [(v * np.sqrt(200.0 * tau / top)).astype(F32) for v in (g, r)]
    if zero_g:
        g[...] = 0.0
    o = Ops(b)
    G, ldg = o.put("g", g, n, pe, pe + 3, 1)
    R, ldr = o.put("r", r, n, pe, pe + 5, 2)
    DG, lddg = o.put("dg", rng.standard_normal((n, pe)).astype(F32), n, pe, pe + 4, 3)
    DR, lddr = o.put("dr", rng.standard_normal((n, pe)).astype(F32), n, pe, pe + 7, 5)
    b.arr("loss", np.full(1, 3.0, F32))
    b.arr("ws", np.zeros(n + 1024, F32))
    res = {}
    for k, (has_g, acc_g, has_r, acc_r, acc_l) in enumerate(NCE_STEPS):
        b.run("nce_loss", G, ldg, R, ldr, n, p, e, tau, weight, "loss", acc_l, DG if has_g else None, lddg, acc_g,
              DR if has_r else None, lddr, acc_r, "ws")
        res[f"loss{k}"] = fetch(b, "loss")
        res[f"dg{k}"], res[f"dr{k}"] = o.get("dg"), o.get("dr")
    return res


# ---- whole-tensor l2 normalisation
L2N_TOL = {"y": (1e-5, 1e-7), "stat": (1e-5, 1e-7), "dx": (1e-4, 1e-6)}  # test_l2norm_parts / _segments
L2N_C = 2
# rows x c = 8192 x 2 = 16 384 elements: the last size of the register kernel; 8193 x 2: the looping kernel
L2N_CASES = [(entry, rows, special) for entry in ("one", "parts", "segs") for rows in (37, 8192, 8193)
             for special in (False, True)]
# f32_error (floor 0: relative to max|spec|) of the near-clamp part (sum x^2 between 1.05e-12 and 1.5e-12), largest
# over y / stat / dx and the L2N_CASES
L2N_TINY_F32_ERR = 1.45e-7


def l2n_shape(entry):
    return (1, 1) if entry == "one" else (3, 1) if entry == "parts" else (3, 2)


def l2n_kinds(entry, special):
    """what each part holds: 'normal', 'zero' (the clamp: y = 0, stat = [0, 1e6], dx = dy * 1e6) or 'tiny' (just above)"""
    if not special:
        return ["normal"] * l2n_shape(entry)[0]
    return ["tiny"] if entry == "one" else ["zero", "tiny", "normal"]


def run_l2norm(b, entry, rows, special, kinds=None):
    """-> per part p: y{p}, dxa{p} (accumulate = 1 on a pre-filled dx), dxo{p} (accumulate = 0), stat{p} [segs x 2]"""
    parts, segs = l2n_shape(entry)
    kinds = kinds or l2n_kinds(entry, special)
    c, R = L2N_C, segs * rows
    rng = np.random.default_rng(_seed("l2n", entry, rows, kinds))
    x = (rng.standard_normal((R, parts * c)) * (1 + np.arange(R)[:, None] // rows)).astype(F32)
    for p, kind in enumerate(kinds):
        if kind == "zero":
            x[:, p * c:(p + 1) * c] = 0.0
        elif kind == "tiny":
            x[:, p * c:(p + 1) * c] = (np.sqrt(1.05e-12 / (rows * c)) * rng.choice([-1.0, 1.0], (R, c)) *
                                       (1 + 0.19 * rng.random((R, c)))).astype(F32)
    w = parts * c
    o = Ops(b)
    X, ldx = o.put("x", x, R, w, w + 3, 1)
    Y, ldy = o.put("y", None, R, w, w + 6, 2)
    DY, lddy = o.put("dy", rng.standard_normal((R, w)).astype(F32), R, w, w + 5, 3)
    dx0 = rng.standard_normal((R, w)).astype(F32)
    b.arr("stat", np.full(2 * parts * segs + 8, SENT, F32))
    mid = {"one": (), "parts": (parts,), "segs": (parts, segs)}[entry]
    name = {"one": "l2norm", "parts": "l2norm_parts", "segs": "l2norm_segs"}[entry]
    b.run(name + "_fwd", X, ldx, rows, c, *mid, Y, ldy, "stat")
    res = {}
    st = fetch(b, "stat")
    for arr in st:
        assert (bits(arr[2 * parts * segs:]) == bits(SENT)).all(), "stat: written past the last part"
    y = o.get("y")
    got = {"y": y}
    for key, acc in (("dxa", 1), ("dxo", 0)):
        DX, lddx = o.put("dx", dx0, R, w, w + 8, 4)
        b.run(name + "_bwd", X, ldx, DY, lddy, rows, c, *mid, "stat", DX, lddx, acc)
        got[key] = o.get("dx")
    for p in range(parts):
        for key, pair in got.items():
            res[f"{key}{p}"] = tuple(v[:, p * c:(p + 1) * c] for v in pair)
        for j, key in enumerate(("ss", "inv")):
            res[f"{key}{p}"] = tuple(v[:2 * parts * segs].reshape(segs, parts, 2)[:, p, j] for v in st)
    res["_dy"] = (o.get("dy")[0], dx0)
    return res


def check_l2norm(b, entry, rows, special):
    res = run_l2norm(b, entry, rows, special)
    dy, dx0 = res.pop("_dy")
    for p, kind in enumerate(l2n_kinds(entry, special)):
        sub = {k: v for k, v in res.items() if k.endswith(str(p))}
        if kind == "tiny":
            for k, (h, e) in sub.items():
                assert_close_rel(f"l2norm {entry} rows={rows} near the clamp: {k}", h, e, L2N_TINY_F32_ERR)
            assert (sub[f"ss{p}"][0] > 1e-12).all() and (sub[f"ss{p}"][0] < 2e-12).all()
            continue
        close_all(sub, {"y": L2N_TOL["y"], "ss": L2N_TOL["stat"], "inv": L2N_TOL["stat"], "dx": L2N_TOL["dx"]},
                  f"l2norm {entry} rows={rows} {kind}:")
        if kind == "zero":
            cols = slice(p * L2N_C, (p + 1) * L2N_C)
            assert (sub[f"y{p}"][0] == 0).all() and (sub[f"ss{p}"][0] == 0).all()
            np.testing.assert_allclose(sub[f"inv{p}"][0], 1e6, rtol=1e-6)
            np.testing.assert_allclose(sub[f"dxo{p}"][0], dy[:, cols] * np.float32(1e6), rtol=1e-6)
            np.testing.assert_allclose(sub[f"dxa{p}"][0], dx0[:, cols] + dy[:, cols] * np.float32(1e6), rtol=1e-6, atol=1e-6)


# ---- tfgan losses: hypel_gan_loss and hypel_loss_terms_slots + hypel_loss_finalize_slots
LOSS_SHAPES = [(rows, c) for rows in (1, 300, 3000) for c in (1, 37, 300)]
GAN_LOSS_TOL = {"loss": (1e-5, 1e-5), "da": (1e-5, 1e-7), "db": (1e-5, 1e-8)}  # test_gan_losses_l2norm_nce
SLOTS_TOL = {"loss": (2e-5, 1e-6), "": (1e-5, 1e-6)}  # test_loss_terms_slots
L2_LONG = 300001  # more than one pass of 1024 blocks x 256 threads
# f32_error of the regulariser term over L2_LONG weights, accumulated three times onto a loss of 3 (loss) / onto dw
L2_LONG_F32_ERR = dict(loss=1.32e-7, dw=0.0)  # (dw: below one ulp, the floor of measured_tol applies)


def loss_operands(rng, rows, c):
    a = rng.standard_normal((rows, c)).astype(F32)
    bb = rng.standard_normal((rows, c)).astype(F32)
    tie = rng.random((rows, c)) < 1.0 / 3  # a == b exactly: the L1 gradient there is 0
    if rows * c >= 3:
        tie.reshape(-1)[0] = True
    bb[tie] = a[tie]
    return a, bb


def run_gan_loss(b, mode, rows, c):
    """three accumulating rounds onto a loss of 3, then one that overwrites it; da / db present, absent, both flags"""
    rng = np.random.default_rng(_seed("gan_loss", mode, rows, c))
    a, bb = loss_operands(rng, rows, c)
    o = Ops(b)
    A, lda = o.put("a", a, rows, c, c + 3, 1)
    Bb, ldb = o.put("bb", bb, rows, c, c + 5, 2)
    DA, ldda = o.put("da", rng.standard_normal((rows, c)).astype(F32), rows, c, c + 4, 3)
    DB, lddb = o.put("db", rng.standard_normal((rows, c)).astype(F32), rows, c, c + 7, 5)
    b.arr("loss", np.full(1, 3.0, F32))
    b.arr("ws", np.zeros(rows + 4096, F32))
    res = {}
    for k, (has_a, acc_a, has_b, acc_b, acc_l) in enumerate([(1, 0, 1, 1, 1), (1, 1, 0, 0, 1), (0, 0, 1, 0, 1), (1, 1, 1, 1, 0)]):
        b.run("gan_loss", mode, A, lda, Bb if mode == 1 else None, ldb, rows, c, 1.0, 0.5, "loss", acc_l,
              DA if has_a else None, ldda, acc_a, DB if has_b and mode == 1 else None, lddb, acc_b, "ws")
        res[f"loss{k}"], res[f"da{k}"], res[f"db{k}"] = fetch(b, "loss"), o.get("da"), o.get("db")
    if mode == 1:
        assert (a == bb).mean() > 0.2 or rows * c < 3
    return res


def run_loss_slots(b, rows, c, nw=5000, only_l2=False):
    """One launch of five terms over one arena (least squares; L1 with both gradients, flags 1 / 0; L1 with db only;
    Wasserstein without gradients; l2 regulariser), three rounds, the loss accumulated onto 3."""
    rng = np.random.default_rng(_seed("slots", rows, c, nw))
    a, bb = loss_operands(rng, rows, c)
    spec = [("a0", rng.standard_normal((rows, c)).astype(F32), c + 3, 1), ("a1", a, c + 5, 2), ("b1", bb, c + 4, 3),
            ("a2", rng.standard_normal((rows, c)).astype(F32), c + 7, 5), ("da0", rng.standard_normal((rows, c)).astype(F32), c + 2, 1),
            ("da1", rng.standard_normal((rows, c)).astype(F32), c + 9, 4), ("db1", rng.standard_normal((rows, c)).astype(F32), c + 6, 0),
            ("db4", rng.standard_normal((rows, c)).astype(F32), c + 8, 7)]
    ar, off, pos = {}, {}, 0
    chunks = []
    for nm, data, ld, col in spec:
        ar[nm] = Arena(rows, c, ld, col, data)
        off[nm] = pos + ar[nm].off
        chunks.append(ar[nm].buf)
        pos += ar[nm].buf.size
    wpos = pos + 16
    wv = (rng.standard_normal(nw) * 0.5).astype(F32)
    dwv = rng.standard_normal(nw).astype(F32)
    chunks += [np.full(16, SENT, F32), wv, np.full(16, SENT, F32), dwv, np.full(16, SENT, F32)]
    dwpos = wpos + nw + 16
    N, cnt = LOSS_NONE, float(rows * c)
    ld = {nm: ar[nm].ld for nm in ar}
    terms = [
        (off["a0"], N, off["da0"], N, ld["a0"], 0, ld["da0"], 0, rows, 0, c, 0, 0, 1.0, 0.5 / cnt, 0.5 / cnt, 0),
        (off["a1"], off["b1"], off["da1"], off["db1"], ld["a1"], ld["b1"], ld["da1"], ld["db1"], rows, 1, c, 1, 0, 0.0,
         10.0 / cnt, 10.0 / cnt, 1),
        (off["a1"], off["b1"], N, off["db4"], ld["a1"], ld["b1"], 0, ld["db4"], rows, 1, c, 0, 1, 0.0, 2.0 / cnt, 2.0 / cnt, 4),
        (off["a2"], N, N, N, ld["a2"], 0, 0, 0, rows, 2, c, 0, 0, 0.0, 1.0 / cnt, 1.0 / cnt, 2),
        (wpos, N, dwpos, N, 0, 0, 0, 0, nw, 3, 1, 1, 0, 0.0, 1e-3, 0.5e-3, 3)]
    if only_l2:
        terms = [terms[-1][:-1] + (0,)]
    n_slots = 1 if only_l2 else 5
    b.arr("arena", np.concatenate(chunks))
    b.arr("terms", np.array(terms, LOSS_TERM_DTYPE))
    b.arr("slots", np.full(n_slots * 1024 + 8, SENT, F32))
    b.arr("loss", np.full(1, 3.0, F32))
    for _ in range(3):
        b.run("loss_terms_slots", "arena", "terms", len(terms), "slots")
        b.run("loss_finalize_slots", "slots", n_slots, "loss", 1)
    res = {"loss": fetch(b, "loss")}
    full = fetch(b, "arena")
    slots = fetch(b, "slots")
    pos = 0
    for nm, data, _, _ in spec:
        size = ar[nm].buf.size
        for v, who in zip(full, ("", " (spec)")):
            ar[nm].check(v[pos:pos + size], nm + who)
        res[nm] = tuple(ar[nm].window(v[pos:pos + size]).copy() for v in full)
        if only_l2 or nm[0] != "d":  # operands that no term of this launch writes keep their bits
            assert_same_bits(nm + " is an input", res[nm][0], data)
        pos += size
    for v in full + slots:
        tail = v[n_slots * 1024:] if v.size == n_slots * 1024 + 8 else np.concatenate(
            [v[wpos - 16:wpos], v[wpos + nw:dwpos], v[dwpos + nw:]])
        assert (bits(tail) == bits(SENT)).all(), "guards around w / dw / the slots"
    assert_same_bits("w is an input", full[0][wpos:wpos + nw], wv)
    res["dw"] = tuple(v[dwpos:dwpos + nw].copy() for v in full)
    return res
