"""-m gpu: the slab reduces of csrc/elementwise.hip through the C ABI -- hypel_reduce_splits_f32, _pair, _multi,
_multi_sized, _wave_multi -- and hypel_act_bias_bwd_reduce, on the case table of tests/reduce_cases.py.

Per case: (1) the device allocation equals, bit for bit, the allocation in which every live output holds its form's
float32 twin -- the documented summation order -- and every other float (sentinels before, between and behind the
operands, the gaps of a window, the partial slabs, the bias) what it held before; (2) independently of the order, every
output lies within the derived bound (m - 1) U sum |terms| of the float64 sum; (3) a second launch on fresh copies gives
the same bits; then the equivalences include/hypel.h states, the argument refusals, and the known answers.  No bound
here comes from what the device produced; tests/test_reduce_cases_emu.py holds the twins to the same bounds on the CPU.
The worst observed error / bound per form is printed at the end (-s)."""
import numpy as np
import pytest

from hypelcnn_amd.backend import HypelError, Ref
from tests import bn_ref as R
from tests import reduce_cases as C
from tests.parity_util import bits

pytestmark = pytest.mark.gpu

F32 = np.float32
WORST = {}       # form -> [worst error / bound, error, bound] against the float64 definition
ACT_WORST = {}   # (form, quantity) -> worst error / bound of hypel_act_bias_bwd_reduce


@pytest.fixture(scope="module")
def hip():
    from hypelcnn_amd.backend import HipBackend
    yield HipBackend()
    print("\nslab reduces: worst |device - float64 definition| / derived bound per kernel form")
    for form in C.FORMS:
        if form in WORST:
            ratio, err, bound = WORST[form]
            print(f"  reduce form {form:10s} ratio {ratio:7.4f}   error {err:.3e}   bound {bound:.3e}")
    for (form, what), ratio in sorted(ACT_WORST.items()):
        print(f"  act_bias_bwd_reduce {form:6s} {what:8s} ratio {ratio:7.4f}")


def _same_allocation(name, got, want):
    if not np.array_equal(bits(got), bits(want)):
        C.same_bits_or_nan(name, got, want)


@pytest.mark.parametrize("case", C.SMALL, ids=repr)
def test_case_bits_bound_sentinels_and_replay(hip, case):
    built = case.build()
    buf, bias = built.run(hip, check_base=True)
    C.hold_to_definition(built, buf, WORST)                                    # (2), whatever the order
    _same_allocation(f"{case.name}: device against the {case.forms} twin", buf, built.expected())   # (1) and (3)
    assert np.array_equal(bits(bias), bits(built.bias0)), "the bias was written"
    buf2, _ = built.run(hip)
    assert np.array_equal(bits(buf2), bits(buf)), "a second launch on fresh copies gives other bits"
    if case.answer:
        C.check_answer(built, buf)


@pytest.mark.parametrize("case", C.BIG, ids=repr)
def test_grid_tail(hip, case):
    """one output past one grid pass of a form, and the count that just fits: integers, so the twin is the exact sum"""
    built = case.build()
    want = built.expected()
    for launch in range(2):
        buf, _ = built.run(hip, check_base=True)
        _same_allocation(f"{case.name} launch {launch}", buf, want)
    for op in built.live():
        WORST.setdefault(op.form, [0.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------------- the equivalences
def _as_separate_f32(hip, built):
    t = hip.upload(built.buf0)
    for op in built.live():
        hip.call("reduce_splits_f32", Ref(t, op.p_off), op.stride, op.S, Ref(t, op.o_off), op.count, op.acc, None, 0, 0)
    hip.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("case", [c for c in C.CASES if c.entry == "reduce_splits_pair_f32"], ids=repr)
def test_pair_equals_two_single_launches(hip, case):
    built = case.build()
    _same_allocation(case.name, built.run(hip)[0], _as_separate_f32(hip, built))


@pytest.mark.parametrize("case", [c for c in C.CASES if c.entry == "reduce_splits_multi_sized_f32"], ids=repr)
def test_sized_table_equals_the_table(hip, case):
    built = case.build()
    sized = built.run(hip)[0]
    built.entry = "reduce_splits_multi_f32"
    _same_allocation(case.name, sized, built.run(hip)[0])


@pytest.mark.parametrize("case", [c for c in C.CASES if " shift0" in c.name], ids=repr)
def test_aligned_base_equals_the_base_one_element_further(hip, case):
    a, b = case.build(), C.by_name(case.name.replace(" shift0", " shift1")).build()
    ga, gb = a.run(hip)[0], b.run(hip)[0]
    for oa, ob in zip(a.ops, b.ops):
        assert (oa.S, oa.count, oa.acc) == (ob.S, ob.count, ob.acc) and oa.p_off % 4 == 0 and ob.p_off % 4 == 1
        assert np.array_equal(bits(oa.take(a.buf0, oa.p_off)), bits(ob.take(b.buf0, ob.p_off)))      # the same data
        got_a, got_b = oa.take(ga, oa.o_off), ob.take(gb, ob.o_off)
        assert np.array_equal(bits(got_a), bits(got_b)), f"{case.name}: {oa.form} at the aligned base, {ob.form} one element further"


# --------------------------------------------------------------------------------------------------- the refusals
def test_argument_refusals_write_nothing(hip):
    built = C.by_name("f32 S5 window n8 ldc16 bias acc1 shift0").build()
    op = built.ops[0]
    t, bt = hip.upload(built.buf0), hip.upload(built.bias0)
    et = hip.upload(built.entries())
    p, o, b = Ref(t, op.p_off), Ref(t, op.o_off), Ref(bt, op.b_off)
    refused = [("reduce_splits_f32", (p, op.stride, 0, o, op.count, 1, None, 0, 0)),             # n_splits < 1
               ("reduce_splits_f32", (p, op.stride, -3, o, op.count, 0, None, 0, 0)),
               ("reduce_splits_f32", (p, op.stride, op.S, o, -1, 1, None, 0, 0)),                # count < 0
               ("reduce_splits_f32", (p, op.stride, op.S, o, op.count, 1, b, 0, 0)),             # a bias without n > 0
               ("reduce_splits_f32", (p, op.stride, op.S, o, op.count, 0, None, 0, 16)),         # a window without n > 0
               ("reduce_splits_f32", (p, op.stride, op.S, o, op.count, 0, b, -8, 16)),
               ("reduce_splits_pair_f32", (p, op.stride, 0, o, p, op.stride, 8, o, op.S, 1)),    # count0 == 0
               ("reduce_splits_pair_f32", (p, op.stride, 8, o, p, op.stride, 0, o, op.S, 0)),
               ("reduce_splits_pair_f32", (p, op.stride, 8, o, p, op.stride, 8, o, 0, 1)),       # n_splits < 1
               ("reduce_splits_multi_sized_f32", (Ref(t), Ref(et), 1, -1)),                      # max_count < 0
               ("reduce_splits_multi_f32", (Ref(t), Ref(et), -1)),
               ("reduce_splits_wave_multi_f32", (Ref(t), Ref(et), 1, -1))]
    for name, args in refused:
        with pytest.raises(HypelError, match="invalid argument"):
            hip.call(name, *args)
    hip.synchronize()
    assert np.array_equal(bits(t.cpu().numpy()), bits(built.buf0)) and np.array_equal(bits(bt.cpu().numpy()), bits(built.bias0))
    # what the contract allows and defines as nothing to do
    hip.call("reduce_splits_f32", p, op.stride, op.S, o, 0, 1, None, 0, 0)
    hip.call("reduce_splits_multi_f32", Ref(t), Ref(et), 0)
    hip.call("reduce_splits_multi_sized_f32", Ref(t), Ref(et), 1, 0)
    hip.call("reduce_splits_wave_multi_f32", Ref(t), Ref(et), 1, 0)
    hip.synchronize()
    assert np.array_equal(bits(t.cpu().numpy()), bits(built.buf0))


# ======================================================================================== hypel_act_bias_bwd_reduce
def _ratio(key, err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    ACT_WORST[key] = max(ACT_WORST.get(key, 0.0), float(r.max()))


@pytest.mark.parametrize("rows,c,chunk", C.ACT_SHAPES)
def test_act_bias_bwd_reduce(hip, rows, c, chunk):
    """bn_act_bwd_reduce_kernel<VEC, true>: dy bit for bit where the derivative is a constant per branch (none, leaky
    ReLU, ReLU; the kink values y == 0, -0, +-1e-30 are planted), within bn_ref's bound for sigmoid and tanh; both rows of
    every chunk record and the finalised dparam within bn_ref's bounds; sentinels; replay; float4 against scalar on dy."""
    y, dz, mask = C.act_inputs(rows, c)
    dp0 = np.random.default_rng(c).standard_normal(c).astype(np.float32)
    for act in C.ACTS:
        for use_mask in (False, True):
            m = mask if use_mask else None
            twin = C.act_dy_twin(dz, y, act, m)
            dys = {}
            for v4 in (True, False):
                for in_place in (False, True):
                    ar = C.act_layout(rows, c, v4, in_place)
                    form = C.act_form(ar, c)
                    assert form == ("v4" if v4 and c % 4 == 0 else "scalar")
                    what = f"act {act} mask {use_mask} {form} in_place {in_place}"
                    ref = C.act_reference(dz, y, act, m, chunk, form)
                    got = C.act_run(hip, ar, rows, c, act, use_mask, chunk, y, dz, mask, dp0)
                    if twin is not None:
                        assert np.array_equal(bits(got["dy"]), bits(twin)), f"dy: {what}"
                    err = np.abs(got["dy"] - ref["dyh"])
                    _ratio((form, "dy"), err, ref["e_dyh"])
                    assert (err <= ref["e_dyh"]).all(), f"dy outside the derived bound: {what}"
                    err = np.abs(got["part"] - ref["part"])
                    _ratio((form, "partial"), err, ref["e_part"])
                    assert (err <= ref["e_part"]).all(), f"partial outside the derived bound: {what}"
                    for acc in (0, 1):
                        want = ref["s0"] + (dp0 if acc else 0.0)
                        bound = ref["e_s0"] + (R.MARGIN * R.rnd(want) if acc else 0.0)
                        err = np.abs(got["dparam"][acc] - want)
                        _ratio((form, "dparam"), err, bound)
                        assert (err <= bound).all(), f"dparam accumulate {acc} outside the merged bound: {what}"
                    again = C.act_run(hip, ar, rows, c, act, use_mask, chunk, y, dz, mask, dp0)
                    assert all(np.array_equal(bits(got[k]), bits(again[k])) for k in ("dy", "part")), f"replay: {what}"
                    dys[(form, in_place)] = got["dy"]
            first = next(iter(dys.values()))
            assert all(np.array_equal(bits(first), bits(d)) for d in dys.values()), f"act {act} mask {use_mask}: dy differs between {list(dys)}"
            assert {f for f, _ in dys} == ({"v4", "scalar"} if c % 4 == 0 else {"scalar"})
