"""CPU: the case table of tests/reduce_cases.py without a device.  Every case selects the kernel form it names, every
form's float32 twin lies within the derived bound of the float64 definition, the emulation (EmuBackend.k_reduce_splits_*)
agrees with the definition within the same bound and leaves every sentinel alone, the known answers hold for the twins,
the table covers what the device test relies on, and the checks refuse planted defects.  The same for the cases of
hypel_act_bias_bwd_reduce against tests/bn_ref.py."""
import numpy as np
import pytest

from tests import bn_ref as R
from tests import reduce_cases as C
from tests.emu_backend import EmuBackend
from tests.parity_util import SENT, bits

F32 = np.float32


def _outside_untouched(built, buf, bias):
    """only the live outputs of the allocation may differ from before the launch"""
    changed = bits(buf) != bits(built.buf0)
    for op in built.live():
        op.put(changed, op.o_off, False)
    assert not changed.any(), f"{built.case.name}: {int(changed.sum())} floats outside the live outputs were written"
    assert np.array_equal(bits(bias), bits(built.bias0)), f"{built.case.name}: the bias was written"


@pytest.mark.parametrize("case", C.SMALL, ids=repr)
def test_case_selects_its_form_twin_and_emulation_within_the_bound(case):
    built = case.build()                                  # asserts the selection and that the operands are normal
    assert tuple(op.form for op in built.ops) == case.forms
    want = built.expected()
    C.hold_to_definition(built, want, what="twin")
    buf, bias = built.run(EmuBackend())
    C.hold_to_definition(built, buf, what="emulation")
    _outside_untouched(built, buf, bias)
    _outside_untouched(built, want, built.bias0)
    for op in built.live():                               # accumulate == 0 onto NaN: every live output is overwritten
        if not op.plant:
            assert np.isfinite(op.take(want, op.o_off)).all() and np.isfinite(op.take(buf, op.o_off)).all()
    if case.answer:
        C.check_answer(built, want)


@pytest.mark.parametrize("case", C.BIG, ids=repr)
def test_grid_tail_cases_have_one_exact_sum(case):
    """small integers: the twin of every order, the emulation and the float64 sum are the same floats"""
    built = case.build()
    want = built.expected()
    buf, _ = built.run(EmuBackend())
    assert np.array_equal(bits(buf), bits(want))
    for op in built.live():
        slabs, bias, old = built.terms(op)
        assert bias is None
        exact = slabs.sum(0, dtype=np.float64) + (0.0 if old is None else old)
        assert np.array_equal(op.take(want, op.o_off).astype(np.float64), exact)
        assert C.twin_table(slabs[:, :4096], None, None if old is None else old[:4096]).tolist() == exact[:4096].tolist()


def test_the_bound_holds_for_all_four_orders():
    """S over every switch of the kernels, magnitudes spread over six decades per slab, with and without the old value:
    each order's float32 result within (m - 1) U sum |terms| of the exact sum; the worst ratio is printed (-s)."""
    worst = {}
    for S in (1, 15, 16, 17, 32, 63, 64, 65, 113, 128, 129, 241, 300):
        rng = np.random.default_rng(S)
        slabs = (rng.standard_normal((S, 4000)) * 10.0 ** rng.uniform(-3, 3, (S, 4000))).astype(np.float32)
        old = (rng.standard_normal(4000) * 10.0 ** rng.uniform(-3, 3, 4000)).astype(np.float32)
        C.assert_normal(slabs, "bound"), C.assert_normal(old, "bound")
        for o in (None, old):
            exact, bound = C.definition(slabs, None, o)
            for name, twin in (("flat", C.twin_flat), ("table", C.twin_table), ("wave", C.twin_wave), ("wave_multi", C.twin_wave_multi)):
                err = np.abs(twin(slabs, None, o).astype(np.float64) - exact)
                assert (err <= bound).all(), (name, S)
                if bound.min() > 0:
                    worst[name] = max(worst.get(name, 0.0), float((err / bound).max()))
    print("\nworst float32 twin error / derived bound:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0


def test_the_orders_differ_where_their_comments_say_so():
    """the cancellation answer: slabs first and the old value last gives w, the old value first gives fl(fl(w + v) - v)"""
    v, w = F32(C.CANCEL_V), F32(C.CANCEL_W)
    slabs = np.zeros((40, 3), np.float32)
    slabs[3], slabs[21] = v, -v
    old = np.full(3, w, np.float32)
    for twin in (C.twin_flat, C.twin_wave, C.twin_wave_multi):
        assert (twin(slabs, None, old) == w).all()
    assert (C.twin_table(slabs, None, old) == F32(C.TABLE_CANCEL)).all() and F32(C.TABLE_CANCEL) == (w + v) - v != w
    nz = np.full((3, 2), -0.0, np.float32)
    for twin in (C.twin_flat, C.twin_wave, C.twin_wave_multi, C.twin_table):
        assert not np.signbit(twin(nz)).any()
    assert np.signbit(C.twin_table(nz, None, nz[0])).all() and not np.signbit(C.twin_flat(nz, None, nz[0])).any()
    # the butterfly is a tree, not a chain: 64 slabs of which one is large
    s = np.full((64, 1), F32(1.0))
    s[0] = F32(2.0 ** 24)
    assert C.twin_wave(s)[0] == F32(2.0 ** 24) + F32(32.0) + F32(16.0) + F32(8.0) + F32(4.0) + F32(2.0) + F32(0.0) != C.twin_flat(s)[0]
    # and the table launch of the wave kind has an order of its own (16 groups through LDS, no butterfly): group 0 loses
    # its three ones to 2^24, the other fifteen groups bring four each
    assert C.twin_wave_multi(s)[0] == F32(2.0 ** 24) + F32(60.0) != C.twin_wave(s)[0]
    assert C.twin_flat(s)[0] == C.twin_table(s)[0] == F32(2.0 ** 24)


def test_the_table_covers_what_it_claims():
    per_entry = {e: [c for c in C.CASES if c.entry == e] for e in C.ENTRIES}
    assert all(per_entry.values())
    selected = {f for c in C.CASES for f in c.forms if f}
    assert selected == set(C.FORMS)
    assert {(name, side) for c in C.BIG for name, side in [c.cap]} == {(f, s) for f in ("flat", "flat4", "table", "table4", "wave_multi")
                                                                      for s in ("over", "under")}
    by = {c.name: c for c in C.CASES}
    assert by["tail flat over"].ops[0].count == 2097152 + 333 and by["tail flat4 over"].ops[0].count == 8388608 + 8
    assert by["tail table over"].ops[0].count == 196608 + 5 and by["tail table4 over"].ops[0].count == 786432 + 4
    assert by["tail wave_multi over"].ops[0].count == 262144 + 70 and by["tail wave_multi over"].ops[0].S == 17
    assert sum(op.count for op in by["tail wave_multi under"].ops) == 262144
    assert C.FLAT_PASS - 4 < by["tail flat under"].ops[0].count <= C.FLAT_PASS and by["tail flat4 under"].ops[0].count == 4 * C.FLAT_PASS
    assert C.TABLE_PASS - 4 < by["tail table under"].ops[0].count <= C.TABLE_PASS and by["tail table4 under"].ops[0].count == 4 * C.TABLE_PASS
    assert C.WAVE_PASS == 8192 and by["f32 S32 n8193 wave passes"].ops[0].count == C.WAVE_PASS + 1

    def shapes(entry, form):
        return {(op.S, op.count) for c in per_entry[entry] for op, f in zip(c.ops, c.forms) if f == form}

    f32 = C.ENTRIES[0]
    assert shapes(f32, "flat") >= {(S, n) for S in C.FLAT_S for n in C.COUNTS} | {(32, 65537)}
    assert shapes(f32, "flat4") >= {(S, n) for S in C.FLAT_S for n in C.COUNTS if n % 4 == 0}
    assert shapes(f32, "wave") >= {(S, n) for S in C.WAVE_S for n in C.COUNTS} | {(32, 8192), (32, 8193), (32, 65536)}
    assert shapes(C.ENTRIES[4], "wave_multi") >= {(S, n) for S in C.WAVE_MULTI_S for n in C.COUNTS}
    assert {S for S, _ in shapes(C.ENTRIES[1], "wave_pair")} >= {32, 64, 65} and {S for S, _ in shapes(C.ENTRIES[1], "flat")} >= {31}
    assert ("flat", "wave") in {c.forms for c in per_entry[C.ENTRIES[1]]}          # one count above 65 536
    for e in C.ENTRIES:                                                             # accumulate 0 and 1 everywhere
        assert {op.acc for c in per_entry[e] for op in c.ops} == {0, 1}
    for e in C.ENTRIES[2:4]:
        assert any(len(c.ops) == 300 for c in per_entry[e]) and any(0 in [op.count for op in c.ops] for c in per_entry[e])
        assert any({"table", "table4"} <= set(c.forms) for c in per_entry[e])
    first_mid_last = by["wave_multi boundaries and empty entries"].ops
    assert first_mid_last[0].count == 0 and first_mid_last[-1].count == 0 and any(op.count == 0 for op in first_mid_last[1:-1])
    sized = by["sized misaligned largest entry"]
    big = max(sized.ops, key=lambda op: op.count)
    assert sized.forms[sized.ops.index(big)] == "table" and -(-big.count // C.SIZED_ITEMS_PER_BLOCK) * 256 * 4 < 2 * big.count
    variants = [op for c in per_entry[f32] for op in c.ops]
    assert {(op.n % 4 == 0) for op in variants if op.bias} == {True, False} and any(op.bias and op.n == 7 for op in variants)
    assert {(op.n % 4 == 0) for op in variants if op.ldc > 0} == {True, False}
    assert any(op.ldc > 0 and op.count % op.n for op in variants)


def test_the_checks_refuse_planted_defects():
    built = C.by_name("f32 S9 n65 acc1 shift1").build()
    want = built.expected()
    op = built.ops[0]
    C.hold_to_definition(built, want)
    bad = want.copy()
    bad[op.o_off + 7] *= F32(1.001)
    with pytest.raises(AssertionError, match="derived bound"):
        C.hold_to_definition(built, bad)
    bad = want.copy()
    bad[op.o_off + 7] = np.nextafter(bad[op.o_off + 7], F32(np.inf))
    with pytest.raises(AssertionError, match="differ in their bits"):
        C.same_bits_or_nan("planted", bad, want)
    for where in (op.o_off - 1, op.o_off + op.count, op.p_off + 3, 0, want.size - 1):
        bad = want.copy()
        bad[where] = F32(1.0)
        with pytest.raises(AssertionError, match="differ in their bits"):
            C.same_bits_or_nan("planted", bad, want)
        with pytest.raises(AssertionError, match="were written"):
            _outside_untouched(built, bad, built.bias0)
    # a window's gaps are outside its live outputs
    built = C.by_name("f32 S5 ragged window n7 ldc13 acc0 shift1").build()
    op = built.ops[0]
    assert bits(built.buf0[op.o_off + 7]) == bits(SENT) and bits(built.buf0[op.o_off + 4 * 13 + 6]) != bits(SENT)
    assert bits(built.buf0[op.o_off + 8 * 13 + 4]) == bits(SENT) and np.isnan(built.buf0[op.o_off + 8 * 13 + 3])
    # a table twin where the flat one belongs is told apart by the known answer
    built = C.by_name("cancel flat").build()
    bad = built.buf0.copy()
    op = built.ops[0]
    op.put(bad, op.o_off, C.twin_table(*built.terms(op)))
    with pytest.raises(AssertionError, match="known answer"):
        C.check_answer(built, bad)
    with pytest.raises(AssertionError, match="selects"):
        C.Case("planted", C.ENTRIES[0], [C.Op(32, 8)], ["flat4"], 0).build()
    with pytest.raises(AssertionError, match="below 2\\^-100"):
        C.assert_normal(np.array([1e-40], np.float32), "planted")


# ============================================================================================ hypel_act_bias_bwd_reduce
@pytest.mark.parametrize("rows,c,chunk", C.ACT_SHAPES)
def test_act_bias_cases_on_the_emulation_and_the_float32_twin(rows, c, chunk):
    y, dz, mask = C.act_inputs(rows, c)
    dp0 = np.random.default_rng(c).standard_normal(c).astype(np.float32)
    nch = (rows + chunk - 1) // chunk
    seen = set()
    for v4 in (True, False):
        for in_place in (False, True):
            ar = C.act_layout(rows, c, v4, in_place)
            form = C.act_form(ar, c)
            assert form == ("v4" if v4 and c % 4 == 0 else "scalar")
            seen.add(form)
            lds = [ar[k].ld for k in ("dz", "y", "mask")] + ([] if in_place else [ar["dy"].ld])
            assert len(set(lds)) == len(lds)
            for act in C.ACTS:
                for use_mask in (False, True):
                    m = mask if use_mask else None
                    ref = C.act_reference(dz, y, act, m, chunk, form)
                    got = C.act_run(EmuBackend(), ar, rows, c, act, use_mask, chunk, y, dz, mask, dp0)
                    assert (np.abs(got["dy"] - ref["dyh"]) <= ref["e_dyh"]).all()
                    assert (np.abs(got["part"] - ref["part"]) <= ref["e_part"]).all()
                    for acc in (0, 1):
                        want = ref["s0"] + (dp0 if acc else 0.0)
                        assert (np.abs(got["dparam"][acc] - want) <= ref["e_s0"] + (R.MARGIN * R.rnd(want) if acc else 0.0)).all()
                    twin = C.act_dy_twin(dz, y, act, m)
                    if twin is not None:                   # plain float32 in the kernel's structure meets the bounds too
                        assert (np.abs(twin - ref["dyh"]) <= ref["e_dyh"]).all()
                        assert (np.abs(C.act_partial_twin(dz, y, act, m, chunk, form) - ref["part"]) <= ref["e_part"]).all()
                        assert got["part"].shape == (nch, 2, c)
    assert seen == ({"v4", "scalar"} if c % 4 == 0 else {"scalar"})


def test_act_bias_inputs_hold_the_kink_values():
    y, dz, mask = C.act_inputs(300, 64)
    assert (y == 0).any() and np.signbit(y[y == 0]).any() and (y == F32(1e-30)).any() and (y == F32(-1e-30)).any()
    t = C.act_dy_twin(dz, y, R.ACT_LRELU, None)
    assert np.array_equal(bits(t[y == 0]), bits((dz[y == 0] * F32(C.ALPHA)).astype(np.float32)))   # slope alpha AT the kink
    assert np.array_equal(bits(t[y == F32(1e-30)]), bits(dz[y == F32(1e-30)]))
    assert (C.act_dy_twin(dz, y, R.ACT_RELU, None)[y <= 0] == 0).all() and C.act_dy_twin(dz, y, R.ACT_TANH, None) is None
