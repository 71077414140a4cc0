"""CPU: the bounds of tests/bn_ref.py are neither false nor empty.  On every data family the fp32 twin of the statistics
kernels stays inside them, each of three naive ways to compute the same statistics leaves them on a named family, and
the float64 definitions agree with tests/emu_backend.py on the easy family (the two specifications cannot drift)."""
import numpy as np
import pytest
import torch

from hypelcnn_amd.backend import Ref
from tests import bn_ref as R
from tests.emu_backend import EmuBackend

EPS, DECAY = 1e-3, 0.95
# (rows, chunk_rows, form): many small chunks with a one-row last chunk (a merge of 257 records), the 256-row chunks of
# the product in the scalar form, and the one-chunk short-matrix form
SHAPES = [(4097, 16, "v4"), (2049, 256, "scalar"), (993, 993, "small")]
COLS = 24  # four columns of each family


def _outside(got, want, bound):
    with np.errstate(invalid="ignore"):
        return ~(np.abs(np.asarray(got, np.float64) - want) <= bound)


def _run(x, chunk_rows, form, partials, merge):
    """Which columns leave a bound anywhere along partials -> merged mean / M2 / rstd."""
    rows = x.shape[0]
    lanes = R.FORMS[form][0]
    ns = R.chunk_sizes(rows, chunk_rows)
    mk, qk = partials(x, chunk_rows, lanes)
    mk_d, qk_d = R.partials_def(x, chunk_rows)
    sb = R.stats_bounds(x, chunk_rows, form, EPS, DECAY)
    bad = _outside(mk, mk_d, sb["part_mean"]).any(0) | _outside(qk, qk_d, sb["part_m2"]).any(0)
    mean, m2 = merge(mk, qk, ns)
    mean_d, m2_d, _ = R.stats_def(x)
    fin = R.finish_def(mean, m2, rows, EPS)
    fin_d = R.finish_def(mean_d, m2_d, rows, EPS)
    bad |= _outside(R.F32(mean), mean_d, sb["mean"]) | _outside(R.F32(m2), m2_d, sb["m2"])
    bad |= _outside(R.F32(fin["rstd"]), fin_d["rstd"], sb["rstd"])
    return bad


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}")
def case(request):
    rows, chunk_rows, form = request.param
    x, fam = R.family_matrix(rows, COLS, chunk_rows, seed=rows)
    x.setflags(write=False)
    return x, fam, chunk_rows, form


def test_twin_stays_inside_the_bounds_on_every_family(case):
    x, fam, chunk_rows, form = case
    bad = _run(x, chunk_rows, form, R.twin_partials, R.merge64)
    assert not bad.any(), f"families outside: {sorted(set(fam[bad]))}"


def test_twin_is_exact_on_the_constant_and_alternating_families(case):
    x, fam, chunk_rows, form = case
    mk, qk = R.twin_partials(x, chunk_rows, R.FORMS[form][0])
    assert (mk[:, fam == "b"] == R.F32(3.25)).all() and (qk[:, fam == "b"] == 0).all()
    if R.sums_exact(x.shape[0], chunk_rows):
        mk_d, qk_d = R.partials_def(x, chunk_rows)
        e = fam == "e"
        assert np.array_equal(mk[:, e], mk_d[:, e].astype(np.float32))
        assert np.array_equal(qk[:, e], qk_d[:, e].astype(np.float32))


# the family on which each naive twin must leave the bounds (at the 4097 x 16 and 2049 x 256 shapes):
#   sum of squares:  c -- x^2 ~ 1e8 has an ulp of 8 while the chunk's M2 is ~ n * 0.01
#   unshifted sum:   c -- the running sum of n values near 1e4 rounds at n * 1e4 * U per addition, the shifted one at
#                    0.1 * U; both errors land in the chunk means whose SPREAD (0.1 / sqrt(n)) is what M2 is made of
#   fp32 merge:      c -- n_k mean_k^2 ~ 1e9 has an ulp of 64 or more while the merged M2 is ~ N * 0.01
NAIVE = {"sumsq": (R.naive_partials_sumsq, R.merge64, "c"),
         "unshifted": (R.naive_partials_unshifted, R.merge64, "c"),
         "merge32": (R.twin_partials, R.naive_merge32, "c")}


@pytest.mark.parametrize("name", sorted(NAIVE))
def test_each_naive_twin_leaves_the_bounds_on_its_family(name):
    partials, merge, family = NAIVE[name]
    hits = []
    for rows, chunk_rows, form in SHAPES[:2]:
        x, fam = R.family_matrix(rows, COLS, chunk_rows, seed=rows)
        bad = _run(x, chunk_rows, form, partials, merge)
        hits.append(sorted(str(f) for f in set(fam[bad])))
        print(f"{name} at {rows} x {chunk_rows} ({form}): outside on families {hits[-1]}")
    assert any(family in h for h in hits), f"{name} stays inside the bounds on family {family}: {hits}"


def test_bounds_are_small_where_the_data_is_easy():
    """Not empty in the other direction either: on N(0, 1) the bound on rstd is below 1e-5 relative, tighter than the
    rtol = 1e-5 the emulation comparison allows, and on the constant family it is one rounding of 1 / sqrt(eps)."""
    x, fam = R.family_matrix(4097, COLS, 16, seed=4097)
    sb = R.stats_bounds(x, 16, "v4", EPS)
    _, m2, _ = R.stats_def(x)
    r = R.finish_def(0, m2, 4097, EPS)["rstd"]
    assert (sb["rstd"][fam == "a"] / r[fam == "a"] < 1e-5).all()
    assert (sb["rstd"][fam == "b"] <= 2.1 * R.U * r[fam == "b"] * R.SLACK).all()


def test_definitions_agree_with_the_emulation_on_the_easy_family():
    """Statistics, moving averages, forward and backward of the definitions against EmuBackend on N(0, 1) data: both
    are float64, so they agree to float64 rounding of the operations and the float32 rounding of what the emulation
    stores (mean / rstd are stored as float32 and reused by its forward)."""
    rows, c, chunk = 777, 12, 128
    rng = np.random.default_rng(7)
    x, _ = R.family_matrix(rows, c, chunk, seed=5, fams="a")
    emu = EmuBackend()
    up = lambda a: emu.upload(np.asarray(a, np.float32))
    nch = (rows + chunk - 1) // chunk
    t = {"x": up(x), "part": up(np.zeros(nch * 2 * c)), "mean": up(np.zeros(c)), "rstd": up(np.zeros(c))}
    mm0, mv0 = rng.standard_normal(c).astype(np.float32), (rng.random(c) + 0.5).astype(np.float32)
    t["mm"], t["mv"] = up(mm0), up(mv0)
    emu.call("col_stats_partial", Ref(t["x"]), c, rows, c, chunk, Ref(t["part"]))
    emu.call("bn_finalize", Ref(t["part"]), nch, chunk, rows, c, EPS, Ref(t["mean"]), Ref(t["rstd"]), Ref(t["mm"]),
             Ref(t["mv"]), DECAY)
    mk, qk = R.partials_def(x, chunk)
    part = t["part"].numpy().reshape(nch, 2, c)
    np.testing.assert_allclose(part[:, 0], mk, rtol=2e-7, atol=1e-7)
    np.testing.assert_allclose(part[:, 1], qk, rtol=2e-7)
    mean, m2, _ = R.stats_def(x)
    fin = R.finish_def(mean, m2, rows, EPS, mm0, mv0, DECAY)
    for k in ("mean", "rstd", "mm", "mv"):
        np.testing.assert_allclose(t[k].numpy(), fin[k], rtol=3e-7, atol=1e-7, err_msg=k)
    # forward / backward with the emulation's own stored statistics
    mean32, rstd32 = t["mean"].numpy().copy(), t["rstd"].numpy().copy()
    beta = (rng.standard_normal(c) * 0.1).astype(np.float32)
    dz = rng.standard_normal((rows, c)).astype(np.float32)
    mask = ((rng.random((rows, c)) < 0.7) / 0.7).astype(np.float32)
    res = rng.standard_normal((rows, c)).astype(np.float32)
    t.update(beta=up(beta), dz=up(dz), mask=up(mask), res=up(res), z=up(np.zeros(rows * c)), dy=up(np.zeros(rows * c)),
             sums=up(np.zeros(2 * c)), dp=up(np.ones(c)), bpart=up(np.zeros(nch * 2 * c)))
    for act in range(5):
        emu.call("bn_act_fwd", Ref(t["x"]), c, rows, c, Ref(t["mean"]), Ref(t["rstd"]), Ref(t["beta"]), act, 0.18,
                 Ref(t["mask"]), c, Ref(t["res"]), c, None, None, 0, None, Ref(t["z"]), c)
        z = R.fwd_def(x, mean32, rstd32, beta, act, 0.18, mask, (res,))
        np.testing.assert_allclose(t["z"].numpy().reshape(rows, c), z, rtol=3e-7, atol=1e-7)
        emu.call("bn_act_bwd_reduce", Ref(t["dz"]), c, Ref(t["x"]), c, rows, c, Ref(t["mean"]), Ref(t["rstd"]),
                 Ref(t["beta"]), act, 0.18, Ref(t["mask"]), c, chunk, Ref(t["bpart"]))
        t["dp"].fill_(1.0)
        emu.call("bwd_reduce_finalize", Ref(t["bpart"]), nch, c, Ref(t["sums"]), Ref(t["dp"]), 1)
        emu.call("bn_act_bwd_apply", Ref(t["dz"]), c, Ref(t["x"]), c, rows, c, Ref(t["mean"]), Ref(t["rstd"]),
                 Ref(t["beta"]), act, 0.18, Ref(t["mask"]), c, Ref(t["sums"]), Ref(t["dy"]), c)
        d = R.bwd_def(dz, x, mean32, rstd32, beta, act, 0.18, mask)
        sums = t["sums"].numpy().reshape(2, c)
        scale = np.abs(d["dyh"]).sum(0)
        assert (np.abs(sums[0] - d["s0"]) <= 3e-7 * scale).all() and (np.abs(sums[1] - d["s1"]) <= 1e-6 * scale).all()
        assert (np.abs(t["dp"].numpy() - (1.0 + d["s0"])) <= 3e-7 * (1 + scale)).all()
        np.testing.assert_allclose(t["dy"].numpy().reshape(rows, c), d["dy"], rtol=1e-5, atol=1e-6)
    # the multi-rank merge IS the statistics of the concatenated rows
    parts = [x[:300], x[300:301], x[301:]]
    recs = [R.stats_def(p) for p in parts]
    mean_m, m2_m = R.merge64([r[0] for r in recs], [r[1] for r in recs], [p.shape[0] for p in parts])
    np.testing.assert_allclose(mean_m, mean, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(m2_m, m2, rtol=1e-12)
    assert isinstance(t["x"], torch.Tensor)
