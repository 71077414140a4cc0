"""TEST INFRASTRUCTURE (no device code): the slab reduces of csrc/elementwise.hip -- hypel_reduce_splits_f32, _pair,
_multi, _multi_sized, _wave_multi -- and the no-batch-norm backward reduce hypel_act_bias_bwd_reduce, written down as

1. float32 TWINS, one per kernel form: exactly the additions the kernel's comment documents, one rounding per
   addition, each order in one function (`twin_flat`, `twin_table`, `twin_wave`, `twin_wave_multi`).  A change of a
   kernel's order edits one of them.
2. the DEFINITION: the exact sum of the m terms of an output (S slabs, a bias if present, the old value if
   accumulating) in float64, whatever the order, and its BOUND (m - 1) * 2^-24 * sum |terms| * SLACK: each of the m - 1
   additions rounds a partial sum that is no larger than sum |terms|.  Nothing in it is measured.  Operands are kept
   normal (asserted on the inputs), so that flushing cannot enter a twin comparison.
3. a CASE TABLE.  A case names its entry point, its reductions (slab count, output count, flags, bias, window, the
   element shift of each base) and the kernel form every reduction must select; `select` derives the form from the
   conditions of the launch code and the placement, and `Case.build` fails when the two differ.  All operands of a case
   are windows of ONE sentinel-filled allocation (parity_util.SENT): `expected` is that allocation with the live outputs
   replaced by the twin, so one bit comparison of the whole allocation covers the outputs, the gaps of a window, the
   floats between the slabs and the partial slabs themselves.

tests/test_reduce_cases_emu.py runs the table on the CPU (twins and the emulation against the definition),
tests/test_gpu_reduce.py on the device."""
import zlib

import numpy as np

from hypelcnn_amd.backend import REDUCE_ENTRY_DTYPE, Ref
from tests import bn_ref as R
from tests.parity_util import SENT, Arena, bits

F32 = np.float32
U = R.U
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]  # what an output holds before an accumulate == 0 launch
LEAD, GAP = 64, 12                                            # sentinel floats before the first and between two regions

# ---- the switches and grid caps, from the launch code of csrc/elementwise.hip (not exported by the library)
WAVE_MIN_SPLITS, WAVE_MAX_COUNT = 32, 65536  # hypel_reduce_splits_f32 / _pair: n_splits >= 32 && count <= 65536
WAVE_PASS = 2048 * 256 // 64                 # hypel_grid_1d(count * 64, 256): 2048 blocks of four waves, one wave per output
FLAT_PASS = 8192 * 256                       # hypel_grid_1d(count_v, 256, 8192): items (floats, or float4s) per grid pass
TABLE_PASS = 768 * 256                       # hypel_reduce_splits_multi_f32: gx = 768 blocks of 256 per entry
SIZED_ITEMS_PER_BLOCK = 4 * 256              # hypel_reduce_splits_multi_sized_f32: want = ceil(max_count / (4 * 256)) <= 768
RSW_TX, RSW_TY = 64, 16                      # reduce_splits_wave_multi_kernel: 64 outputs x 16 slab groups per block
WAVE_MULTI_PASS = 4096 * RSW_TX              # hypel_reduce_splits_wave_multi_f32: at most 4096 chunks of 64 outputs

FORMS = ("flat", "flat4", "wave", "wave_pair", "table", "table4", "wave_multi")
ENTRIES = ("reduce_splits_f32", "reduce_splits_pair_f32", "reduce_splits_multi_f32", "reduce_splits_multi_sized_f32",
           "reduce_splits_wave_multi_f32")


# ===================================================================================================== float32 twins
def _f32(a):
    return None if a is None else np.asarray(a, np.float32)


def twin_flat(slabs, bias=None, old=None):
    """reduce_splits_kernel / reduce_splits_v4_kernel: s = bias or 0, the slabs k = 0 .. S-1, the old value (0 when not
    accumulating) LAST."""
    slabs = _f32(slabs)
    with np.errstate(all="ignore"):
        s = np.zeros(slabs.shape[1], np.float32) if bias is None else _f32(bias).copy()
        for k in range(slabs.shape[0]):
            s = s + slabs[k]
        return s + (F32(0.0) if old is None else _f32(old))


def twin_table(slabs, bias=None, old=None):
    """reduce_splits_multi_kernel, both branches: s = old or 0 FIRST, then the slabs in k order."""
    assert bias is None
    slabs = _f32(slabs)
    with np.errstate(all="ignore"):
        s = np.zeros(slabs.shape[1], np.float32) if old is None else _f32(old).copy()
        for k in range(slabs.shape[0]):
            s = s + slabs[k]
        return s


def twin_wave(slabs, bias=None, old=None):
    """reduce_splits_wave_kernel / reduce_splits_wave_pair_kernel: lane l sums the slabs l, l + 64, .. ascending from
    0.0f; the xor butterfly with offsets 32, 16, .., 1 (every lane adds its partner's value to its own; lane 0 holds
    the result); + bias; old + s."""
    slabs = _f32(slabs)
    with np.errstate(all="ignore"):
        lanes = np.zeros((64, slabs.shape[1]), np.float32)
        for k in range(slabs.shape[0]):
            lanes[k % 64] = lanes[k % 64] + slabs[k]
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[lane ^ off]
        s = lanes[0]
        if bias is not None:
            s = s + _f32(bias)
        return s if old is None else _f32(old) + s


def twin_wave_multi(slabs, bias=None, old=None):
    """reduce_splits_wave_multi_kernel: group ty sums the slabs ty, ty + 16, .. ascending from 0.0f (the eight-in-flight
    loop adds in the same order); the groups are added 1 .. 15 onto sh[0]; the old value last."""
    assert bias is None
    slabs = _f32(slabs)
    with np.errstate(all="ignore"):
        groups = np.zeros((RSW_TY, slabs.shape[1]), np.float32)
        for k in range(slabs.shape[0]):
            groups[k % RSW_TY] = groups[k % RSW_TY] + slabs[k]
        t = groups[0].copy()
        for g in range(1, RSW_TY):
            t = t + groups[g]
        return t if old is None else _f32(old) + t


TWINS = {"flat": twin_flat, "flat4": twin_flat, "wave": twin_wave, "wave_pair": twin_wave, "table": twin_table,
         "table4": twin_table, "wave_multi": twin_wave_multi}


# ========================================================================================= the definition and its bound
def definition(slabs, bias=None, old=None):
    """(exact float64 sum of the m terms, bound (m - 1) U sum |terms| SLACK), per output.  The float64 sum of m <= a few
    hundred float32 terms is off by at most (m - 1) 2^-53 sum |terms|: 2^-29 of the bound, inside SLACK."""
    terms = [np.asarray(slabs, np.float64)]
    if bias is not None:
        terms.append(np.asarray(bias, np.float64)[None])
    if old is not None:
        terms.append(np.asarray(old, np.float64)[None])
    t = np.concatenate(terms, 0)
    with np.errstate(all="ignore"):
        return t.sum(0), (t.shape[0] - 1) * U * np.abs(t).sum(0) * R.SLACK


def assert_normal(a, what):
    """Every operand is 0 or at least 2^-100 in magnitude: a nonzero partial sum of such terms is a multiple of the
    smallest term's last bit (>= 2^-124), so neither an operand nor a partial sum is subnormal."""
    a = np.asarray(a, np.float32)
    f = a[np.isfinite(a)]
    assert not ((f != 0) & (np.abs(f) < 2.0 ** -100)).any(), f"{what}: an operand below 2^-100"
    assert np.abs(f).sum(dtype=np.float64) < 2.0 ** 100, f"{what}: the operands overflow"


# ================================================================================================== selection (host)
def select_f32(op):
    """hypel_reduce_splits_f32: the wave form for n_splits >= 32 && count <= 65536; otherwise float4 when count % 4 == 0,
    rows_v4(partial, stride), rows_v4(out, ldc > 0 ? ldc : 0) and ((ldc <= 0 && !bias) || n % 4 == 0).  Offsets are
    relative to a 16-byte aligned allocation."""
    if op.S >= WAVE_MIN_SPLITS and op.count <= WAVE_MAX_COUNT:
        return "wave"
    v4 = (op.count % 4 == 0 and op.p_off % 4 == 0 and op.stride % 4 == 0 and op.o_off % 4 == 0
          and (op.ldc % 4 == 0 if op.ldc > 0 else True) and ((op.ldc <= 0 and not op.bias) or op.n % 4 == 0))
    return "flat4" if v4 else "flat"


def select_table(op):
    """reduce_splits_multi_kernel, per entry: count % 4 == 0, stride % 4 == 0, both addresses 16-byte aligned."""
    return "table4" if op.count % 4 == 0 and op.stride % 4 == 0 and op.p_off % 4 == 0 and op.o_off % 4 == 0 else "table"


def select(entry, ops):
    if entry == "reduce_splits_f32":
        return tuple(select_f32(op) for op in ops)
    if entry == "reduce_splits_pair_f32":  # the wave pair when hypel_reduce_splits_f32 would pick the wave form for both
        if ops[0].S >= WAVE_MIN_SPLITS and ops[0].count <= WAVE_MAX_COUNT and ops[1].count <= WAVE_MAX_COUNT:
            return ("wave_pair", "wave_pair")
        return tuple(select_f32(op) for op in ops)
    if entry in ("reduce_splits_multi_f32", "reduce_splits_multi_sized_f32"):
        return tuple(select_table(op) if op.count else None for op in ops)
    assert entry == "reduce_splits_wave_multi_f32"
    return tuple("wave_multi" if op.count else None for op in ops)


# =============================================================================================================== cases
class Op:
    """One reduction of a case.  sp / so: element shift of the partial / output base from a 16-byte boundary; pad: floats
    between the span of one slab and the next (3 makes the stride odd); data: 'spread' (N(0, 1) times 10^U(-3, 3)),
    'ints' (a tiled pattern of integers in [-8, 8]), 'zeros', 'negzero'; old: the value every old output holds (None: of
    the same kind as the data); plant: ('cancel', a, b, v) puts +v / -v into slabs a / b of every output,
    ('nonfinite', k, i, value) puts `value` into slab k at output i."""

    def __init__(self, S, count, acc=0, n=0, ldc=0, bias=False, sp=0, so=0, pad=4, data="spread", old=None, plant=None):
        self.S, self.count, self.acc, self.n, self.ldc, self.bias = int(S), int(count), int(acc), int(n), int(ldc), bool(bias)
        self.sp, self.so, self.pad, self.data, self.old, self.plant = sp, so, pad, data, old, plant
        assert (self.n > 0) or not (self.bias or self.ldc > 0)
        self.span = ((self.count - 1) // self.n * self.ldc + (self.count - 1) % self.n + 1 if self.ldc > 0 else self.count) if self.count else 0
        self.stride = (self.span + 3) // 4 * 4 + pad
        self.p_off = self.o_off = self.b_off = None
        self.form = None

    def index(self):
        """o(i) of include/hypel.h, or None for a dense reduction"""
        if self.ldc <= 0:
            return None
        i = np.arange(self.count)
        return (i // self.n) * self.ldc + i % self.n

    def take(self, buf, off):
        idx = self.index()
        return buf[off:off + self.count] if idx is None else buf[off + idx]

    def put(self, buf, off, values):
        idx = self.index()
        if idx is None:
            buf[off:off + self.count] = values
        else:
            buf[off + idx] = values


def _data(rng, kind, shape):
    size = int(np.prod(shape))
    if kind == "spread":
        return (rng.standard_normal(size) * 10.0 ** rng.uniform(-3, 3, size)).astype(np.float32).reshape(shape)
    if kind == "ints":
        return np.resize(rng.integers(-8, 9, 1009).astype(np.float32), size).reshape(shape)
    return np.full(shape, {"zeros": 0.0, "negzero": -0.0}[kind], np.float32)


class Case:
    """name, entry point, the reductions, the form each must select (None for an entry without outputs), and for the known
    answers `answer`: per reduction None, ('all', value) or ('class', output, 'nan' | '+inf' | '-inf')."""

    def __init__(self, name, entry, ops, forms, seed, answer=None, big=False, cap=None):
        assert entry in ENTRIES and len(ops) == len(forms)
        self.name, self.entry, self.ops, self.forms, self.seed = name, entry, ops, tuple(forms), seed
        self.answer, self.big, self.cap = answer, big, cap   # cap: (threshold name, 'over' | 'under') of a grid-tail case

    def __repr__(self):                                      # the test id
        return self.name.replace(" ", "-")

    def build(self):
        return Built(self)


class Built:
    """The placed and filled operands of a case: `buf0` the allocation before the launch, `bias0` the bias vectors (in a
    sentinel-filled buffer of their own, one element off a 16-byte boundary), `ops` with p_off / o_off / b_off."""

    def __init__(self, case):
        self.case, self.entry, self.ops = case, case.entry, case.ops
        cur = LEAD
        for op in self.ops:
            op.p_off = (cur + 3) // 4 * 4 + op.sp
            cur = op.p_off + (max(op.S - 1, 0) * op.stride + op.span if op.count else 0) + GAP
            op.o_off = (cur + 3) // 4 * 4 + op.so
            cur = op.o_off + op.span + GAP
        self.buf0 = np.full(cur + LEAD, SENT, np.float32)
        rng = np.random.default_rng(case.seed)
        nb, bias_parts = 1, [np.full(1, SENT, np.float32)]
        for op in self.ops:
            if not op.count:
                continue
            slabs = _data(rng, op.data, (op.S, op.count))
            old = _data(rng, op.data, op.count) if op.old is None else np.full(op.count, op.old, np.float32)
            if op.plant and op.plant[0] == "cancel":
                _, a, b, v = op.plant
                slabs[a], slabs[b] = F32(v), -F32(v)
            if op.plant and op.plant[0] == "nonfinite":
                _, k, i, value = op.plant
                slabs[k, i] = value
            assert_normal(slabs, case.name), assert_normal(old, case.name)
            for k in range(op.S):
                op.put(self.buf0, op.p_off + k * op.stride, slabs[k])
            op.put(self.buf0, op.o_off, old if op.acc else QNAN)
            if op.bias:
                b = _data(rng, "ints" if op.data == "ints" else "spread", op.n)
                assert_normal(b, case.name)
                assert (b != 0).all() or op.data == "ints"
                op.b_off = nb
                bias_parts += [b, np.full(3, SENT, np.float32)]
                nb += op.n + 3
        self.bias0 = np.concatenate(bias_parts)
        got = select(self.entry, self.ops)
        assert got == case.forms, f"{case.name}: selects {got}, meant for {case.forms}"
        for op, f in zip(self.ops, got):
            op.form = f

    def terms(self, op):
        """(slabs [S x count], bias per output or None, old per output or None) of a reduction, from buf0"""
        slabs = np.stack([op.take(self.buf0, op.p_off + k * op.stride) for k in range(op.S)])
        bias = np.resize(self.bias0[op.b_off:op.b_off + op.n], op.count) if op.bias else None
        return slabs, bias, (op.take(self.buf0, op.o_off).copy() if op.acc else None)

    def live(self):
        return [op for op in self.ops if op.count]

    def expected(self):
        """the allocation after the launch: every live output replaced by its form's twin, every other float as before"""
        buf = self.buf0.copy()
        for op in self.live():
            op.put(buf, op.o_off, TWINS[op.form](*self.terms(op)))
        return buf

    def entries(self):
        return np.array([(op.p_off, op.o_off, op.stride, op.count, op.S, op.acc) for op in self.ops], REDUCE_ENTRY_DTYPE)

    def run(self, be, check_base=False):
        """Upload fresh copies, launch through `be` (HipBackend or EmuBackend), return (allocation, bias buffer) after."""
        t, bt = be.upload(self.buf0), be.upload(self.bias0)
        if check_base:
            assert Ref(t).ptr() % 16 == 0 and Ref(bt).ptr() % 16 == 0
        ops, at = self.ops, lambda off: Ref(t, off)
        if self.entry == "reduce_splits_f32":
            op, = ops
            be.call(self.entry, at(op.p_off), op.stride, op.S, at(op.o_off), op.count, op.acc,
                    Ref(bt, op.b_off) if op.bias else None, op.n, op.ldc)
        elif self.entry == "reduce_splits_pair_f32":
            a, b = ops
            assert a.S == b.S and a.acc == b.acc
            be.call(self.entry, at(a.p_off), a.stride, a.count, at(a.o_off), at(b.p_off), b.stride, b.count, at(b.o_off), a.S, a.acc)
        else:
            et = be.upload(self.entries())
            extra = {"reduce_splits_multi_f32": (), "reduce_splits_multi_sized_f32": (max(op.count for op in ops),),
                     "reduce_splits_wave_multi_f32": (sum(op.count for op in ops),)}[self.entry]
            be.call(self.entry, at(0), Ref(et), len(ops), *extra)
        be.synchronize()
        return t.cpu().numpy().copy(), bt.cpu().numpy().copy()


def same_bits_or_nan(name, got, want):
    """bit for bit, except where the twin is NaN: there the device value must be a NaN (the payload of a propagated NaN is
    not part of any contract)"""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, name
    nan = np.isnan(want)
    bad = np.flatnonzero(np.where(nan, ~np.isnan(got), bits(got) != bits(want)))
    assert bad.size == 0, (f"{name}: {bad.size} of {got.size} floats differ in their bits; first at element {int(bad[0])}: "
                           f"{got[bad[0]]!r} for {want[bad[0]]!r}")


def hold_to_definition(built, buf, worst=None, what="device"):
    """every finite-defined live output of `buf` within the derived bound of the float64 definition; a non-finite definition
    asks for the same class (NaN, +Inf, -Inf).  worst: {form: [ratio, error, bound]} to update."""
    for j, op in enumerate(built.live()):
        exact, bound = definition(*built.terms(op))
        got = op.take(buf, op.o_off).astype(np.float64)
        fin = np.isfinite(exact)
        g, e = got[~fin], exact[~fin]                          # NaN for NaN, and an infinity of the same sign
        assert (np.isnan(g) == np.isnan(e)).all() and (g[~np.isnan(e)] == e[~np.isnan(e)]).all(), \
            f"{built.case.name} reduction {j}: a non-finite sum did not reach its output"
        err = np.abs(got[fin] - exact[fin])
        bad = ~(err <= bound[fin])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound[fin])
        assert not bad.any(), (f"{built.case.name} reduction {j} ({op.form}, {what}): {int(bad.sum())} outputs outside the derived "
                               f"bound, worst error / bound {ratio.max():.3f}")
        if worst is not None and ratio.size:
            i = int(np.argmax(ratio))
            if ratio[i] > worst.setdefault(op.form, [0.0, 0.0, 0.0])[0]:
                worst[op.form] = [float(ratio[i]), float(err[i]), float(bound[fin][i])]


def check_answer(built, buf):
    """the known answers of a case (Case.answer) on an allocation after the launch"""
    for op, ans in zip(built.ops, built.case.answer or [None] * len(built.ops)):
        if ans is None:
            continue
        got = op.take(buf, op.o_off)
        if ans[0] == "all":
            assert (bits(got) == bits(F32(ans[1]))).all(), f"{built.case.name}: {got[:4]} for the known answer {F32(ans[1])!r}"
        else:
            _, i, cls = ans
            v = got[i]
            assert {"nan": np.isnan(v), "+inf": v == np.inf, "-inf": v == -np.inf}[cls], f"{built.case.name}: {v!r} for {cls}"
            assert np.isfinite(np.delete(got, i)).all(), f"{built.case.name}: a non-finite value reached a neighbour"


# ------------------------------------------------------------------------------------------------------- the table
FLAT_S, WAVE_S = (1, 2, 7, 8, 9, 31), (32, 63, 64, 65, 128, 129, 300)
WAVE_MULTI_S = (1, 15, 16, 17, 112, 113, 128, 129, 240, 241, 256)
COUNTS = (1, 3, 4, 5, 63, 64, 65, 900)
TABLE_S = (1, 2, 7, 8, 9, 31, 32, 65)
CANCEL_V, CANCEL_W = 1e4, 1e-3
TABLE_CANCEL = 0.0009765625   # fl(fl(w + v) - v): the table form adds the old value FIRST
F32E, PAIR, MULTI, SIZED, WMULTI = ENTRIES


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _cases():
    out = []

    def add(name, entry, ops, forms, key, **kw):
        out.append(Case(name, entry, ops, forms, _seed(key), **kw))

    # ---- hypel_reduce_splits_f32: slab counts x counts, at an aligned base and one element further (the same data)
    for S in FLAT_S + WAVE_S:
        for ci, count in enumerate(COUNTS):
            for shift in (0, 1):
                acc = (ci + S) % 2
                form = "wave" if S >= 32 else ("flat4" if shift == 0 and count % 4 == 0 else "flat")
                add(f"f32 S{S} n{count} acc{acc} shift{shift}", F32E, [Op(S, count, acc, sp=shift, so=shift)], [form], ("f32", S, count))
    for count in (8192, 8193, 65536):  # one grid pass of the wave form, one output more, the last count of the wave form
        add(f"f32 S32 n{count} wave passes", F32E, [Op(32, count, 1, data="ints", pad=0)], ["wave"], ("f32w", count))
    add("f32 S32 n65537 takes a flat form", F32E, [Op(32, 65537, 1, data="ints", pad=0)], ["flat"], "f32 65537")
    add("f32 S32 n65540 takes the float4 form", F32E, [Op(32, 65540, 0, data="ints", pad=0)], ["flat4"], "f32 65540")
    # ---- variants: accumulate, bias (n % 4 == 0 and n == 7), window (ldc > 0; n % 4 == 0 or not; count % n != 0: o(i) of
    # the header is defined for every i < count, the last row of the window is then a partial one), odd stride
    for S, big in ((5, "flat4"), (40, "wave")):
        for acc in (0, 1):
            for shift in (0, 1):
                v4 = big if S >= 32 or shift == 0 else "flat"
                sc = "wave" if S >= 32 else "flat"
                for tag, kw, form in (("bias n8", dict(count=64, n=8, bias=True), v4),
                                      ("bias n7", dict(count=63, n=7, bias=True), sc),
                                      ("window n8 ldc16", dict(count=64, n=8, ldc=16), v4),
                                      ("window n7 ldc13", dict(count=63, n=7, ldc=13), sc),
                                      ("window n8 ldc13", dict(count=64, n=8, ldc=13), sc),
                                      ("ragged window n8 ldc16", dict(count=60, n=8, ldc=16), v4),
                                      ("ragged window n7 ldc13", dict(count=60, n=7, ldc=13), sc),
                                      ("window n8 ldc16 bias", dict(count=64, n=8, ldc=16, bias=True), v4),
                                      ("window n7 ldc9 bias", dict(count=35, n=7, ldc=9, bias=True), sc),
                                      ("odd stride", dict(count=64, pad=3), sc)):
                    add(f"f32 S{S} {tag} acc{acc} shift{shift}", F32E, [Op(S, acc=acc, sp=shift, so=shift, **kw)], [form],
                        ("f32v", S, tag, acc))
    # ---- hypel_reduce_splits_pair_f32
    for S in (31, 32, 63, 64, 65, 129):
        for pi, (c0, c1) in enumerate(((1, 1), (65, 3), (900, 7), (64, 64))):
            for shift in (0, 1):
                acc = (pi + S) % 2
                forms = ["wave_pair"] * 2 if S >= 32 else ["flat4" if shift == 0 and c % 4 == 0 else "flat" for c in (c0, c1)]
                add(f"pair S{S} n{c0}+{c1} acc{acc} shift{shift}", PAIR,
                    [Op(S, c0, acc, sp=shift, so=shift), Op(S, c1, acc, sp=shift, so=shift, pad=8)], forms, ("pair", S, c0, c1))
    for acc in (0, 1):  # one count above 65 536: two hypel_reduce_splits_f32, of which the second still takes the wave form
        add(f"pair S32 n65537+5 acc{acc} falls back", PAIR, [Op(32, 65537, acc, data="ints", pad=0), Op(32, 5, acc, data="ints")],
            ["flat", "wave"], ("pairbig", acc))
        add(f"pair S32 n8+65540 acc{acc} falls back", PAIR, [Op(32, 8, acc, data="ints"), Op(32, 65540, acc, data="ints", pad=0)],
            ["wave", "flat4"], ("pairbig2", acc))
    # ---- the table forms: per launch an aligned and a misaligned entry of the same shape (float4 and scalar)
    for entry, tag in ((MULTI, "multi"), (SIZED, "sized")):
        for S in TABLE_S:
            for ci, count in enumerate(COUNTS):
                acc = (ci + S) % 2
                add(f"{tag} S{S} n{count} acc{acc}", entry, [Op(S, count, acc), Op(S, count, 1 - acc, sp=1, so=1)],
                    ["table4" if count % 4 == 0 else "table", "table"], ("table", S, count))
        add(f"{tag} short and empty entries", entry,
            [Op(3, 3, 1), Op(5, 0), Op(4, 64, 0), Op(2, 1, 1), Op(9, 2, 0, sp=1), Op(7, 0, 1), Op(6, 64, 1, pad=3), Op(6, 64, 1, so=2)],
            ["table", None, "table4", "table", "table", None, "table", "table"], "table short")
        # the K-slice shape: 300 entries of one small tile each
        add(f"{tag} 300 entries of one tile", entry, [Op(3, 128, e % 2, pad=0) for e in range(300)], ["table4"] * 300, "table 300")
    # max_count equal to the largest entry, which is misaligned: the grid (one float4 per thread) holds a quarter of the
    # threads that entry needs, so its loop runs four times
    add("sized misaligned largest entry", SIZED, [Op(3, 5000, 1, sp=1, so=1), Op(3, 64, 0), Op(2, 4996, 0, so=3)],
        ["table", "table4", "table"], "sized 5000")
    # ---- hypel_reduce_splits_wave_multi_f32: the n_entries == 1 walk ...
    for S in WAVE_MULTI_S:
        for ci, count in enumerate(COUNTS):
            acc = (ci + S) % 2
            add(f"wave_multi S{S} n{count} acc{acc}", WMULTI, [Op(S, count, acc, sp=ci % 2, so=(ci + S) % 4)], ["wave_multi"],
                ("wmulti", S, count))
    # ... entry boundaries inside a 64-output chunk, zero-count entries first, in the middle and last, every slab count
    add("wave_multi boundaries and empty entries", WMULTI,
        [Op(5, 0), Op(17, 40, 1), Op(113, 50, 0), Op(3, 0, 1), Op(241, 129, 1, so=1), Op(16, 7, 0), Op(1, 1, 1), Op(9, 0)],
        [None, "wave_multi", "wave_multi", None, "wave_multi", "wave_multi", "wave_multi", None], "wmulti mixed")
    add("wave_multi every slab count in one launch", WMULTI, [Op(S, 37, e % 2, so=e % 4) for e, S in enumerate(WAVE_MULTI_S)],
        ["wave_multi"] * len(WAVE_MULTI_S), "wmulti all S")
    # ---- grid tails: one case just past one grid pass of every form and one that just fits; small integers, so that
    # every order gives the same exact sum
    for side, d in (("over", 1), ("under", 0)):
        kw = dict(data="ints", pad=0)
        # hypel_reduce_splits_f32: hypel_grid_1d(count_v, 256, 8192) -> 8192 * 256 = 2 097 152 floats per pass of the scalar form
        add(f"tail flat {side}", F32E, [Op(2, FLAT_PASS + (333 if d else -3), 1, sp=1, so=1, **kw)], ["flat"], "tail flat",
            big=True, cap=("flat", side))
        # the same cap in float4s: 4 * 2 097 152 = 8 388 608 floats per pass
        add(f"tail flat4 {side}", F32E, [Op(2, 4 * FLAT_PASS + (8 if d else 0), 1, **kw)], ["flat4"], "tail flat4",
            big=True, cap=("flat4", side))
        # hypel_reduce_splits_multi_f32: gx = 768 blocks of 256 threads per entry -> 196 608 floats / 786 432 in float4s
        add(f"tail table {side}", MULTI, [Op(2, TABLE_PASS + (5 if d else -1), 1, sp=1, so=1, **kw), Op(2, 64, 0, **kw)],
            ["table", "table4"], "tail table", big=True, cap=("table", side))
        add(f"tail table4 {side}", MULTI, [Op(2, 4 * TABLE_PASS + (4 if d else 0), 1, **kw), Op(2, 63, 0, **kw)],
            ["table4", "table"], "tail table4", big=True, cap=("table4", side))
        # hypel_reduce_splits_wave_multi_f32: min(chunks, 4096) blocks of 64 outputs -> 262 144 outputs per pass
        wm = [Op(17, WAVE_MULTI_PASS + 70, 1, **kw)] if d else [Op(17, 100000, 1, **kw), Op(17, WAVE_MULTI_PASS - 100000, 0, so=1, **kw)]
        add(f"tail wave_multi {side}", WMULTI, wm, ["wave_multi"] * len(wm), "tail wave_multi", big=True, cap=("wave_multi", side))
    # ---- known answers
    cancel = dict(acc=1, data="zeros", old=CANCEL_W)
    w, tc = ("all", CANCEL_W), ("all", TABLE_CANCEL)
    for shift, f in ((0, "flat4"), (1, "flat")):
        add(f"cancel {f}", F32E, [Op(9, 8, sp=shift, so=shift, plant=("cancel", 2, 7, CANCEL_V), **cancel)], [f], "cancel", answer=[w])
        add(f"cancel table shift{shift}", MULTI, [Op(9, 8, sp=shift, so=shift, plant=("cancel", 7, 2, CANCEL_V), **cancel)],
            ["table" if shift else "table4"], "cancel", answer=[tc])
        add(f"cancel sized shift{shift}", SIZED, [Op(9, 8, sp=shift, so=shift, plant=("cancel", 2, 7, CANCEL_V), **cancel)],
            ["table" if shift else "table4"], "cancel", answer=[tc])
    add("cancel wave across lanes", F32E, [Op(70, 8, plant=("cancel", 3, 68, CANCEL_V), **cancel)], ["wave"], "cancel", answer=[w])
    add("cancel wave within a lane", F32E, [Op(70, 8, plant=("cancel", 69, 5, CANCEL_V), **cancel)], ["wave"], "cancel", answer=[w])
    add("cancel pair", PAIR, [Op(40, 8, plant=("cancel", 0, 39, CANCEL_V), **cancel), Op(40, 3, plant=("cancel", 33, 1, CANCEL_V), **cancel)],
        ["wave_pair"] * 2, "cancel", answer=[w, w])
    add("cancel pair flat", PAIR, [Op(9, 8, plant=("cancel", 0, 8, CANCEL_V), **cancel), Op(9, 3, plant=("cancel", 5, 1, CANCEL_V), **cancel)],
        ["flat4", "flat"], "cancel", answer=[w, w])
    add("cancel wave_multi across groups", WMULTI, [Op(40, 8, plant=("cancel", 1, 18, CANCEL_V), **cancel)], ["wave_multi"], "cancel", answer=[w])
    add("cancel wave_multi within a group", WMULTI, [Op(40, 8, plant=("cancel", 35, 3, CANCEL_V), **cancel)], ["wave_multi"], "cancel", answer=[w])
    for vi, (value, cls) in enumerate(((np.nan, "nan"), (np.inf, "+inf"), (-np.inf, "-inf"))):
        for acc in (0, 1):
            a = [("class", 4, cls)]
            nf = lambda S: dict(acc=acc, plant=("nonfinite", S // 2, 4, value))
            add(f"{cls} flat4 acc{acc}", F32E, [Op(9, 12, **nf(9))], ["flat4"], "nf", answer=a)
            add(f"{cls} flat acc{acc}", F32E, [Op(9, 9, **nf(9))], ["flat"], "nf", answer=a)
            add(f"{cls} wave acc{acc}", F32E, [Op(70, 9, **nf(70))], ["wave"], "nf", answer=a)
            add(f"{cls} pair acc{acc}", PAIR, [Op(70, 9, **nf(70)), Op(70, 5, **nf(70))], ["wave_pair"] * 2, "nf", answer=a * 2)
            add(f"{cls} table acc{acc}", MULTI, [Op(9, 12, **nf(9)), Op(9, 9, **nf(9))], ["table4", "table"], "nf", answer=a * 2)
            add(f"{cls} sized acc{acc}", SIZED, [Op(9, 12, **nf(9)), Op(9, 9, **nf(9))], ["table4", "table"], "nf", answer=a * 2)
            add(f"{cls} wave_multi acc{acc}", WMULTI, [Op(40, 9, **nf(40)), Op(3, 70, **nf(3))], ["wave_multi"] * 2, "nf", answer=a * 2)
    # -0.0 slabs only: every form starts from +0.0f, so the sum is +0.0 -- except the table form onto an old -0.0, which
    # starts from the old value
    for acc, old in ((0, None), (1, -0.0)):
        nz = dict(acc=acc, data="negzero", old=old)
        pz, tz = ("all", 0.0), ("all", -0.0 if acc else 0.0)
        add(f"negzero flat acc{acc}", F32E, [Op(3, 9, **nz)], ["flat"], "nz", answer=[pz])
        add(f"negzero flat4 acc{acc}", F32E, [Op(3, 8, **nz)], ["flat4"], "nz", answer=[pz])
        add(f"negzero wave acc{acc}", F32E, [Op(33, 8, **nz)], ["wave"], "nz", answer=[pz])
        add(f"negzero pair acc{acc}", PAIR, [Op(33, 8, **nz), Op(33, 3, **nz)], ["wave_pair"] * 2, "nz", answer=[pz, pz])
        add(f"negzero table acc{acc}", MULTI, [Op(3, 8, **nz), Op(3, 9, **nz)], ["table4", "table"], "nz", answer=[tz, tz])
        add(f"negzero sized acc{acc}", SIZED, [Op(3, 8, **nz), Op(3, 9, **nz)], ["table4", "table"], "nz", answer=[tz, tz])
        add(f"negzero wave_multi acc{acc}", WMULTI, [Op(1, 8, **nz), Op(17, 9, **nz)], ["wave_multi"] * 2, "nz", answer=[pz, pz])
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _cases()
SMALL = [c for c in CASES if not c.big]
BIG = [c for c in CASES if c.big]


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ======================================================================================== hypel_act_bias_bwd_reduce
ALPHA = 0.18
ACTS = (R.ACT_NONE, R.ACT_LRELU, R.ACT_RELU, R.ACT_SIGMOID, R.ACT_TANH)
# (rows, c, chunk_rows): one element; odd; a ragged last chunk at both chunk lengths; around STAT_TX = 64 columns; three
# column blocks with a last one of four columns
ACT_SHAPES = [(1, 1, 64), (5, 7, 64), (257, 37, 64), (257, 37, 256), (300, 64, 256), (300, 68, 256), (1000, 132, 256)]


def act_inputs(rows, c):
    """(y, dz, mask): y standard normal with the kink values 0, -0, +-1e-30 planted, dz spread over four decades, the mask
    of a dropout with keep 0.7"""
    rng = np.random.default_rng(rows * 131 + c)
    y = rng.standard_normal((rows, c)).astype(np.float32)
    kink = np.array([0.0, -0.0, 1e-30, -1e-30], np.float32)
    flat = y.reshape(-1)
    where = rng.choice(flat.size, size=min(flat.size, max(1, flat.size // 8)), replace=False)
    flat[where] = kink[np.arange(where.size) % 4]
    dz = (rng.standard_normal((rows, c)) * 10.0 ** rng.uniform(-2, 2, (rows, c))).astype(np.float32)
    mask = ((rng.random((rows, c)) < 0.7) / F32(0.7)).astype(np.float32)
    for a in (y, dz, mask):
        assert_normal(a, "act inputs")
        a.setflags(write=False)
    return y, dz, mask


def act_layout(rows, c, v4, in_place):
    """Arenas of dz, y, mask, dy: four leading dimensions, pairwise different, each window at a column offset; all
    multiples of 4 at aligned bases (the float4 form when c % 4 == 0 too), or not (the scalar form).  In place dy is dz."""
    lds, cols = ((c + 4, c + 8, c + 12, c + 16), (4, 0, 8, 12)) if v4 else ((c + 3, c + 6, c + 4, c + 9), (1, 2, 0, 3))
    lds = tuple((ld + 3) // 4 * 4 for ld in lds) if v4 else lds
    names = ("dz", "y", "mask", "dy")
    ar = {nm: Arena(rows, c, ld, col) for nm, ld, col in zip(names, lds, cols)}
    if in_place:
        ar["dy"] = ar["dz"]
    return ar


def act_form(ar, c):
    """launch_bwd_reduce: float4 iff c % 4 == 0 and every operand's base is 16-byte aligned with ld % 4 == 0"""
    return "v4" if c % 4 == 0 and all(a.off % 4 == 0 and a.ld % 4 == 0 for a in ar.values()) else "scalar"


def act_dy_twin(dz, y, act, mask):
    """dy = fl(fl(dz * mask) * act'(y)) for the activations whose derivative is a constant per branch (none, leaky ReLU,
    ReLU: 1, alpha or 0 -- one multiply or two, each rounded once); None for sigmoid and tanh, whose derivative comes from
    the device's exponential and tanh and is held to bn_ref's bound instead."""
    if act not in (R.ACT_NONE, R.ACT_LRELU, R.ACT_RELU):
        return None
    g = np.asarray(dz, np.float32)
    if mask is not None:
        g = g * np.asarray(mask, np.float32)
    slope = {R.ACT_NONE: F32(1.0), R.ACT_LRELU: F32(ALPHA), R.ACT_RELU: F32(0.0)}[act]
    return (g * np.where(np.asarray(y) > 0, F32(1.0), slope).astype(np.float32)).astype(np.float32)


def act_reference(dz, y, act, mask, chunk, form):
    """float64 definitions and derived bounds: dict(dyh, e_dyh [rows x c]; part, e_part [n_chunks x 2 x c]; s0, e_s0 [c])"""
    rows, c = y.shape
    full = R.bwd_bounds(dz, y, None, None, None, act, ALPHA, mask, chunk, form)
    nch = (rows + chunk - 1) // chunk
    part, e_part = np.empty((nch, 2, c)), np.empty((nch, 2, c))
    for k in range(nch):
        sl = slice(k * chunk, min(rows, (k + 1) * chunk))
        bb = R.bwd_bounds(dz[sl], y[sl], None, None, None, act, ALPHA, None if mask is None else mask[sl], chunk, form)
        part[k, 0], part[k, 1] = bb["def"]["s0"], bb["def"]["s1"]
        e_part[k, 0], e_part[k, 1] = bb["s0"], bb["s1"]
    return {"dyh": full["def"]["dy"], "e_dyh": full["dy"], "part": part, "e_part": e_part, "s0": full["def"]["s0"], "e_s0": full["s0"]}


def act_partial_twin(dz, y, act, mask, chunk, form):
    """float32 chunk sums in the kernel's structure (bn_ref._lane_sums: down the row lanes, then across them) for the
    activations with a bit-defined dy"""
    dy = act_dy_twin(dz, y, act, mask)
    rows, c = y.shape
    nch = (rows + chunk - 1) // chunk
    out = np.empty((nch, 2, c), np.float32)
    for k in range(nch):
        sl = slice(k * chunk, min(rows, (k + 1) * chunk))
        out[k, 0] = R._lane_sums(dy[sl], R.FORMS[form][0])
        out[k, 1] = R._lane_sums((dy[sl] * y[sl]).astype(np.float32), R.FORMS[form][0])
    return out


def act_run(be, ar, rows, c, act, use_mask, chunk, y, dz, mask, dp0):
    """Launch hypel_act_bias_bwd_reduce and hypel_bwd_reduce_finalize (accumulate 0 and 1) on fresh uploads.  Returns
    dict(dy [rows x c], part [n_chunks x 2 x c], dparam {0, 1: [c]}) after checking every sentinel."""
    nch = (rows + chunk - 1) // chunk
    host = {"dz": dz, "y": y, "mask": mask}
    bufs, t = {}, {}
    for nm in ("dz", "y", "mask", "dy"):
        a = ar[nm]
        if nm == "dy" and a is ar["dz"]:
            t["dy"] = t["dz"]
            continue
        b = a.buf.copy()
        if nm in host:
            a.window(b)[...] = host[nm]
        bufs[nm], t[nm] = b, be.upload(b)
        assert t[nm].data_ptr() % 16 == 0                 # act_form counts alignment from the allocation
    pa = Arena(nch, 2 * c, 2 * c, 0)
    pt = be.upload(pa.buf)
    be.call("act_bias_bwd_reduce", Ref(t["dz"], ar["dz"].off), ar["dz"].ld, Ref(t["y"], ar["y"].off), ar["y"].ld, rows, c, act,
            ALPHA, Ref(t["mask"], ar["mask"].off) if use_mask else None, ar["mask"].ld, chunk, Ref(pt, pa.off),
            Ref(t["dy"], ar["dy"].off), ar["dy"].ld)
    res = {"dparam": {}}
    for acc in (0, 1):
        sa, da = Arena(1, 2 * c, 2 * c, 0), Arena(1, c, c + 2, 1, dp0)
        st, dt = be.upload(sa.buf), be.upload(da.buf)
        be.call("bwd_reduce_finalize", Ref(pt, pa.off), nch, c, Ref(st, sa.off), Ref(dt, da.off), acc)
        be.synchronize()
        sa.check(st.cpu().numpy(), "sums"), da.check(dt.cpu().numpy(), "dparam")
        res["dparam"][acc] = da.window(dt.cpu().numpy())[0].copy()
    be.synchronize()
    got = {nm: t[nm].cpu().numpy() for nm in t}
    for nm in ("y", "mask") + (("dz",) if ar["dy"] is not ar["dz"] else ()):
        assert np.array_equal(bits(got[nm]), bits(bufs[nm])), f"{nm}: an input was written"
    ar["dy"].check(got["dy"], "dy")
    pg = pt.cpu().numpy()
    pa.check(pg, "partial")
    res["dy"] = ar["dy"].window(got["dy"]).copy()
    res["part"] = pa.window(pg).reshape(nch, 2, c).copy()
    return res
