"""CPU: every case table of tests/head_kernel_cases.py through the executable spec alone (parity_util.SpecOnly), so that
the cases, their sentinels and their references are exercised without a GPU -- and the reference-side conditions of the
bounds: for each bounded quantity the same formula in plain float32 NumPy (the yardstick) must lie within the derived
bound of the float64 reference; its largest error / bound ratio per quantity is printed (-s).  Then: the tables cover
what they claim, and the checks refuse planted defects."""
import numpy as np
import pytest

from tests import head_kernel_cases as H
from tests import parity_util as PU
from tests.emu_backend import EmuBackend
from tests.test_gpu_head_kernels import POWF_ULP, POWF_ULP_MEASURED

WORST = H.Report()  # over the whole module, for the last test's printout


def settle(rep):
    """the yardstick within every bound (the spec side was held to them while the cases ran)"""
    for line in rep.lines():
        print(line)
    for label, (dev_ratio, yard_ratio) in rep.items():
        WORST.note(label, dev_ratio, yard_ratio)
        assert yard_ratio <= 1.0, f"{label}: plain fp32 is at {yard_ratio:.3f} of the derived bound -- the bound is wrong"


@pytest.mark.parametrize("c", H.LAYOUT_C)
def test_layout_cases(c):
    H.run_layout_c(PU.SpecOnly(), c)


def test_layout_second_trip():
    n, p, c = H.LAYOUT_BIG
    assert n * p * c > 2048 * 256
    H.run_layout(PU.SpecOnly(), n, p, c, c + 3, 1)


@pytest.mark.parametrize("c", H.LRN_C)
def test_lrn_cases_and_yardstick(c):
    rep = H.Report()
    H.run_lrn_c(PU.SpecOnly(), rep, c, POWF_ULP)
    settle(rep)


def test_lrn_grid_stride():
    rows, c, radius = H.LRN_BIG
    assert rows * c > 2048 * 256
    rep = H.Report()
    for k, params in enumerate(H.LRN_PARAMS):
        H.run_lrn(PU.SpecOnly(), rep, rows, c, radius, params, k, POWF_ULP)
    settle(rep)


@pytest.mark.parametrize("shape", H.MSE_SHAPES + [H.MSE_FLAT_BIG], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mse_cases_and_yardstick(shape):
    rep = H.Report()
    H.run_mse(PU.SpecOnly(), rep, *shape, forms=H.MSE_FORMS if shape != H.MSE_FLAT_BIG else [H.MSE_FORMS[0], H.MSE_FORMS[7]])
    settle(rep)


@pytest.mark.parametrize("kind", ["one", "span"])
@pytest.mark.parametrize("shape", [(16, 16), (1, 257)], ids=["flat4", "general"])
def test_mse_one_term_and_wide_span(shape, kind):
    rep = H.Report()
    H.run_mse(PU.SpecOnly(), rep, *shape, kind=kind, forms=[H.MSE_FORMS[0], H.MSE_FORMS[8]])
    settle(rep)


def test_sum_cases_and_yardstick():
    rep = H.Report()
    for count in H.SUM_COUNTS:
        rng = np.random.default_rng(count)
        H.run_sum(PU.SpecOnly(), rep, (rng.standard_normal(count) * 10.0 ** rng.uniform(-2, 2, count)).astype(np.float32), f"n{count}")
    H.run_sum(PU.SpecOnly(), rep, H.sum_pairs_in_chain(np.random.default_rng(1)), "pairs in chain", exact_zero=True)
    H.run_sum(PU.SpecOnly(), rep, H.sum_pairs_across_blocks(np.random.default_rng(2)), "pairs across blocks")
    settle(rep)


@pytest.mark.parametrize("c", H.ARGMAX_C)
def test_argmax_cases(c):
    H.run_argmax_c(PU.SpecOnly(), c)


def test_confusion_one_cell():
    H.run_confusion_one_cell(PU.SpecOnly())


def test_argmax_rule_of_the_header():
    """[1, NaN, 3] -> 2, [NaN, 5] -> 0, all NaN -> 0, +0 / -0 tie -> the first: reference and emulation alike"""
    from tests.emu_backend import _first_max
    z = np.asarray([[1, np.nan, 3], [np.nan, 5, 1], [np.nan] * 3, [-1, -0.0, 0.0], [-1, 0.0, -0.0], [-np.inf] * 3], np.float32)
    assert list(H.first_max(z)) == list(_first_max(z)) == [2, 0, 0, 1, 1, 0]
    assert list(np.argmax(z, 1))[:2] == [1, 0]  # what numpy.argmax would say to the first row: the first NaN


def test_ignored_labels_do_not_reach_the_table():
    b = PU.SpecOnly()
    z = np.zeros((4, 3), np.float32)
    C = H.IntGuard(9, init=np.zeros(9, np.int32))
    b.arr("z", z), b.arr("lab", np.asarray([-1, 3, 255, 2], np.int32)), b.arr("conf", C.buf)
    b.run("argmax_confusion", "z", 3, 4, 3, "lab", None, ("conf", C.off))
    got = H.dev(b, "conf")
    C.check(got, "confusion")
    assert list(C.payload(got)) == [0, 0, 0, 0, 0, 0, 1, 0, 0]


@pytest.mark.parametrize("cc,cl", H.GATHER_CC_CL)
def test_gather_cases(cc, cl):
    for p in (1, 3):
        for n in (1, 6):
            H.run_gather(PU.SpecOnly(), cc, cl, p, n)


def test_gather_block_walk():
    n, p = H.GATHER_BIG
    assert n * p * p > 8192
    H.run_gather(PU.SpecOnly(), 92, 3, p, n)


@pytest.mark.parametrize("nb", [0, 1, 2, 3])
def test_gather_2x_cases(nb):
    H.run_gather_2x(PU.SpecOnly(), nb, 5, 1)
    H.run_gather_2x(PU.SpecOnly(), nb, 94, 2)
    H.run_gather_2x(PU.SpecOnly(), nb, 190, 2, n=1)


def test_gather_2x_reference_is_the_loaders():
    """`loader_patch_2x` against GRSS2018DataSet.get_data_point on a data set built from the same rasters"""
    from hypelcnn_amd.loader.GRSS2018DataLoader import GRSS2018DataSet
    rng = np.random.default_rng(3)
    for nb in (0, 1, 2, 3):
        ds = GRSS2018DataSet.__new__(GRSS2018DataSet)
        ds.neighborhood = nb
        ds.casi = rng.standard_normal((3 + 2 * nb, 4 + 2 * nb, 5)).astype(np.float32)
        ds.lidar = rng.standard_normal((6 + 2 * nb, 7 + 2 * nb, 1)).astype(np.float32)
        for x, y in ((0, 0), (1, 0), (0, 1), (1, 1), (6, 5), (5, 4)):
            np.testing.assert_array_equal(H.loader_patch_2x(ds.casi, ds.lidar, nb, x, y), ds.get_data_point(x, y))


@pytest.mark.parametrize("c", H.AUGMENT_C)
def test_augment_cases(c):
    H.run_augment_c(PU.SpecOnly(), c)


def test_augment_refuses_ratio_with_alt():
    assert "shadow_ratio and shadow_alt" in H.run_augment_refusal(EmuBackend())


@pytest.mark.parametrize("cin", H.CHANMAP_CIN)
@pytest.mark.parametrize("table", [True, False], ids=["table", "identity"])
def test_chanmap_cases_and_yardstick(cin, table):
    rep = H.Report()
    for rows in H.CHANMAP_ROWS:
        for layout in ("aligned", "odd"):
            for accumulate in (0, 1):
                H.run_chanmap(PU.SpecOnly(), rep, cin, rows, layout, accumulate, table)
    settle(rep)


def test_copy_cases():
    H.run_copy_blocks(PU.SpecOnly())
    H.run_copy_pair(PU.SpecOnly())


# ------------------------------------------------------------------------------------------------ the tables, the checks
def test_tables_cover_what_they_claim():
    assert set(H.LAYOUT_C) >= {1, 63, 64, 65, 145, 192, 193, 360, 190}
    for c in H.LAYOUT_C:
        assert set(H.layout_lds(c)) == {c, c + 1, c + 3, c // 4 * 4 + 4}
    assert {n * p for n, p in H.LAYOUT_NP} == {1, 3, 4, 5, 17}
    assert set(H.LRN_C) == {1, 5, 11, 12, 384} and set(H.LRN_RADIUS) == {0, 5, "c"} and set(H.LRN_ROWS) == {1, 3, 257}
    assert {r * c for r, c in H.MSE_SHAPES} >= {1, 3, 4, 255, 256, 257, 1024 * 256 + 4} and {r * c % 4 for r, c in H.MSE_SHAPES} == {0, 1, 2, 3}
    assert H.MSE_FLAT_BIG[0] * H.MSE_FLAT_BIG[1] == 4 * 1024 * 256 + 8
    assert {cc + cl for cc, cl in H.GATHER_CC_CL} == {95, 96, 191, 192, 193} and {cl for _, cl in H.GATHER_CC_CL} == {0, 1, 3}
    assert set(POWF_ULP) == {(float(np.float32(p[2])), k) for p in H.LRN_PARAMS for k in ("fwd", "bwd")}
    assert all(POWF_ULP[k] == 2.0 * v for k, v in POWF_ULP_MEASURED.items())
    rng = np.random.default_rng(0)
    for first in range(5):  # a single row is of the regime it is asked for: zero, or one entry of 1e15, ...
        x, reg = H.lrn_rows(1, 11, first, rng)
        assert reg[0] == first and (np.abs(x).max() > 9e14) == (first == 4) and (not x.any()) == (first == 3)
    z, kind = H.argmax_rows(129, 20, 0, rng)
    assert set(kind) == set(range(len(H.ROW_KINDS))) and np.isnan(z[kind == 14]).all() and np.isnan(z[kind == 11, 0]).all()
    c, start = H.chanmap_table(60)
    d = np.diff(start)
    assert start[0] == 0 and start[-1] == c and (d >= 0).all() and (d == 0).sum() == 3 and d.max() == 33 and len(d) == 60


def test_the_checks_refuse_planted_defects():
    rep = H.Report()
    with pytest.raises(AssertionError, match="derived bound"):
        H.hold(rep, "planted", np.float32(1.0) + np.float32(2.0 ** -20), 1.0, 4 * H.U, 1.0)
    with pytest.raises(AssertionError, match="derived bound"):
        H.hold(rep, "planted zero", np.float32(1e-30), 0.0, 0.0, 0.0)  # a bound of 0 means exact
    with pytest.raises(AssertionError, match="derived bound"):
        H.hold(rep, "planted nan", np.float32(np.nan), 1.0, 1.0, 1.0)
    w = H.Win(3, 5, 8, 1, lead=1)
    w.check(w.buf)
    for where in (w.off - 1, w.off + 5, w.off + 2 * 8 + 5, w.buf.size - 1, 0):
        bad = w.buf.copy()
        bad[where] = np.nextafter(PU.SENT, np.float32(0))
        with pytest.raises(AssertionError, match="were written"):
            w.check(bad)
    g = H.IntGuard(4)
    bad = g.buf.copy()
    bad[g.off + 4] = 0
    with pytest.raises(AssertionError, match="written outside"):
        g.check(bad, "planted")


def test_zz_print_the_largest_yardstick_ratio():
    label, (_, yard_ratio) = WORST.worst_yardstick()
    print(f"\nlargest fp32 yardstick error / derived bound over all cases: {yard_ratio:.3f} ({label})")
    assert yard_ratio <= 1.0
