"""The one-launch batch norms of the FC tail (bn_act_small_fwd / _bwd) at every block shape their host wrappers
choose from the column count -- 4-channel stripes (c <= 128), 8-channel (c <= 512), 16-channel (c <= 1024) and the
32-channel block --
against the float64 definitions and the derived bounds of tests/bn_ref.py, through the guarded windows of
tests/test_gpu_bn_chain.py (a store outside the live [rows x c] part of a padded matrix is seen bit for bit).

Every shape keeps the summation form FORMS["small"] = (32, 17) bounds: 32 row lanes of 32 rows, lanes 2 j and 2 j + 1
paired, the 16 pair sums added to 0 in order.  The shapes differ only in how many channels share a block, so a
column's results do not depend on the width of the launch it is part of: `test_results_do_not_depend_on_the_stripe_width`
runs the same columns inside launches of all four widths and compares bit for bit."""
import functools

import numpy as np
import pytest

from tests import bn_ref as R
from tests.test_gpu_bn_chain import ALPHA, DECAY, EPS, LEAD_ODD, Win, _bits, _in, _out, _within, hip  # noqa: F401

F32 = np.float32
ROWS = [1024, 1023, 33, 1]
# 1, 3, 4, 5: one 4-channel block and its edge; 8, 9: two blocks / the 8-channel width's edge inside the 4-channel form;
# 15, 33, 45: layers of the model; 128 | 129: last 4-channel and first 8-channel launch; 257: 8-channel stripes with a
# ragged last block; 512 | 513: last 8-channel and first 16-channel launch; 980: 16-channel stripes, ragged last block;
# 1024 | 1025: last 16-channel and first 32-channel launch
COLS = [1, 3, 4, 5, 8, 9, 15, 33, 45, 128, 129, 257, 512, 513, 980, 1024, 1025]
@functools.lru_cache(maxsize=None)
def _inputs(rows, c):
    rng = np.random.default_rng(rows * 10000 + c)
    y, fam = R.family_matrix(rows, c, 256, seed=rows * 10000 + c, fams="abcde")
    d = {"y": y, "dz": rng.standard_normal((rows, c)).astype(np.float32),
         "mask": ((rng.random((rows, c)) < 0.7) / F32(0.7)).astype(np.float32),
         "beta": rng.standard_normal(c).astype(np.float32), "mm0": rng.standard_normal(c).astype(np.float32),
         "mv0": (rng.random(c) + 0.5).astype(np.float32), "dp0": rng.standard_normal(c).astype(np.float32)}
    for a in d.values():
        a.setflags(write=False)
    return d, fam


@pytest.mark.gpu
@pytest.mark.parametrize("c", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_small_batch_norm_at_every_block_shape(hip, rows, c):  # noqa: F811
    """Leaky-ReLU forward and backward, with and without mask, dparam accumulating and not, on rows padded to
    ld = c + 3: statistics, moving averages, z, dy and dbeta within the derived bounds; z without mask is the separately
    rounded fp32 chain bit for bit; a second forward call gives the same bits."""
    d, fam = _inputs(rows, c)
    act, ld = R.ACT_LRELU, c + 3
    y, dz, mask, beta = d["y"], d["dz"], d["mask"], d["beta"]
    yin, dzin, mkin = _in(hip, y, ld, 1), _in(hip, dz, ld, 3), _in(hip, mask, ld, 2)
    bt = Win(hip, beta, 1)
    sb = R.stats_bounds(y, rows, "small", EPS, DECAY)
    mean_d, m2_d, _ = R.stats_def(y)
    fin = R.finish_def(mean_d, m2_d, rows, EPS, d["mm0"], d["mv0"], DECAY)
    e_mm, e_mv = R.moving_bounds(sb, fin["mm"], fin["mv"])
    first = None
    for use_mask in (False, True):
        m = mask if use_mask else None
        mean, rstd = Win(hip, c), Win(hip, c)
        zbits = []
        for _ in range(2):
            mm, mv = Win(hip, d["mm0"]), Win(hip, d["mv0"])
            z = _out(hip, rows, ld, LEAD_ODD)
            hip.call("bn_act_small_fwd", yin.ref, ld, rows, c, EPS, bt.ref, act, ALPHA, mkin.ref if use_mask else None,
                     ld, mean.ref, rstd.ref, mm.ref, mv.ref, DECAY, z.ref, ld)
            hip.synchronize()
            zz = z.mat(rows, ld, c, f"z mask {use_mask}")
            zbits.append((_bits(zz), _bits(mean.read("mean")), _bits(rstd.read("rstd")), _bits(mm.read("mm")),
                          _bits(mv.read("mv"))))
        assert all(np.array_equal(a, b) for a, b in zip(*zbits)), "a second call on the same inputs differs"
        mu, rs = mean.read("mean"), rstd.read("rstd")
        if first is None:
            first = (mu, rs)
            _within(mu, fin["mean"], sb["mean"], fam, "tail mean")
            _within(rs, fin["rstd"], sb["rstd"], fam, "tail rstd")
            _within(mm.read("mm"), fin["mm"], e_mm, fam, "tail mm")
            _within(mv.read("mv"), fin["mv"], e_mv, fam, "tail mv")
            b = fam == "b"
            assert np.array_equal(_bits(mu[b]), _bits(np.full(int(b.sum()), 3.25)))
            assert np.array_equal(_bits(rs[b]), _bits(np.full(int(b.sum()), F32(1.0 / np.sqrt(float(F32(EPS)))))))
            assert np.array_equal(_bits(zz), _bits(R.fwd_f32(y, mu, rs, beta, act, ALPHA))), "z: not the separately rounded pre"
        else:
            assert np.array_equal(_bits(mu), _bits(first[0])) and np.array_equal(_bits(rs), _bits(first[1]))
            _within(zz, R.fwd_def(y, mu, rs, beta, act, ALPHA, m), R.fwd_bound(y, mu, rs, beta, act, ALPHA, m), fam, "tail z")
        bb = R.bwd_bounds(dz, y, mu, rs, beta, act, ALPHA, m, rows, "small")
        for acc in (0, 1):
            dy, dp = _out(hip, rows, ld, LEAD_ODD), Win(hip, d["dp0"])
            hip.call("bn_act_small_bwd", dzin.ref, ld, yin.ref, ld, rows, c, mean.ref, rstd.ref, bt.ref, act, ALPHA,
                     mkin.ref if use_mask else None, ld, dy.ref, ld, dp.ref, acc)
            hip.synchronize()
            _within(dy.mat(rows, ld, c, "dy"), bb["def"]["dy"], bb["dy"], fam, "tail dy")
            want = bb["def"]["s0"] + (d["dp0"] if acc else 0.0)
            _within(dp.read("dparam"), want, bb["s0"] + (R.MARGIN * R.rnd(want) if acc else 0.0), fam, "tail dbeta")
        mean.read("mean"), rstd.read("rstd")
    for w in (yin, dzin, mkin, bt):
        w.read("input")


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
def test_results_do_not_depend_on_the_stripe_width(hip, rows):  # noqa: F811
    """The first 128 columns of one [rows x 1025] matrix as part of a 1025-column launch (32-channel blocks), a 1024-column
    launch (16-channel stripes), a 512-column launch (8-channel stripes) and a 128-column launch (4-channel stripes), same
    leading dimension: mean, rstd, moving averages, z, dy and dbeta of those columns are the same bits in all four."""
    d, _ = _inputs(rows, 1025)
    act, ld, keep = R.ACT_LRELU, 1025 + 3, 128
    yin, dzin, mkin = _in(hip, d["y"], ld, 1), _in(hip, d["dz"], ld, 3), _in(hip, d["mask"], ld, 2)
    bt = Win(hip, d["beta"], 1)
    outs = []
    for c in (1025, 1024, 512, 128):
        mean, rstd, mm, mv = Win(hip, c), Win(hip, c), Win(hip, d["mm0"][:c]), Win(hip, d["mv0"][:c])
        z, dy, dp = _out(hip, rows, ld, LEAD_ODD), _out(hip, rows, ld, LEAD_ODD), Win(hip, d["dp0"][:c])
        hip.call("bn_act_small_fwd", yin.ref, ld, rows, c, EPS, bt.ref, act, ALPHA, mkin.ref, ld, mean.ref, rstd.ref,
                 mm.ref, mv.ref, DECAY, z.ref, ld)
        hip.call("bn_act_small_bwd", dzin.ref, ld, yin.ref, ld, rows, c, mean.ref, rstd.ref, bt.ref, act, ALPHA, mkin.ref,
                 ld, dy.ref, ld, dp.ref, 1)
        hip.synchronize()
        outs.append([_bits(w.read(n)[:keep]) for w, n in ((mean, "mean"), (rstd, "rstd"), (mm, "mm"), (mv, "mv"), (dp, "dparam"))]
                    + [_bits(z.mat(rows, ld, c, "z")[:, :keep]), _bits(dy.mat(rows, ld, c, "dy")[:, :keep])])
    for other in outs[1:]:
        for name, a, b in zip(("mean", "rstd", "mm", "mv", "dparam", "z", "dy"), outs[0], other):
            assert np.array_equal(a, b), f"{name} depends on the stripe width"
