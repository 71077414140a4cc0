"""CPU (numpy kernel emulation): the activation range / histogram launches on their twin (tests/emu_activation.py) against
the float64 numpy.histogram reference of tests/activation_cases.py; common/device_activation.ActivationTaps on a tiny
HYPELCNN against numpy.histogram over the fetched taps; utilities/nn_layer_activation_graph end to end from a
checkpoint; its refusals; the bin arithmetic; the reference model's taps through the tf_slim facade.  The helpers are
shared with tests/test_gpu_activation.py, which runs the same checks on the device."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import tests.emu_activation  # noqa: F401 -- attaches the twin to EmuBackend
from hypelcnn_amd.backend import ACT_MAX_BINS
from hypelcnn_amd.common.device_activation import ActivationTaps, storage_views, tap_bins, tap_size
from hypelcnn_amd.utilities import nn_layer_activation_graph as tool
from tests import activation_cases as A
from tests.emu_backend import EmuBackend
from tests.test_summary_emu import ALG, run_episode

TAPS = ["spectral_expansion", "spectral_reduction", "spatial", "classification"]
SCENE = "grss2013:h=24:w=30:bands=10:classes=3:samples=0.6"
BATCH = 32


@pytest.fixture(scope="module")
def be():
    return EmuBackend()


# ----------------------------------------------------------------------------- the launches
@pytest.mark.parametrize("name", A.NAMES)
def test_view_cases(be, name):
    c = A.case(name)
    A.check_case(A.run_case(be, c), c)


def check_contention(be, kind):
    values, edges = A.contention(kind)
    got = A.run_case(be, SimpleNamespace(buffer=values, off=0, rows=1 << 10, ld=1 << 12, cols=1 << 12, edges=edges))
    A.check(got, *A.reference(values, edges, True), where=kind)
    assert np.count_nonzero(got["counts"]) == (1 if kind == "one" else 2) and got["outside"] == 0
    return got


@pytest.mark.parametrize("kind", ["one", "two"])
def test_contention(be, kind):
    got = check_contention(be, kind)
    assert got["counts"].max() == (A.N_CONTENTION if kind == "one" else A.N_CONTENTION // 2)
    if kind == "two":  # the extremes of the data are the first and the last edge: the last bin is closed
        assert got["counts"][0] == got["counts"][-1] == A.N_CONTENTION // 2


def check_accumulation(be):
    """two calls into the same outputs equal one call on the concatenation; a range folded over three views is the
    minimum and the maximum of all of them, whatever the order"""
    c = A.case("70000x33_strided")
    n_bins = len(c.edges) - 1
    buf, edges = be.upload(c.buffer), be.upload(c.edges)
    out = A.fresh_outputs(be, n_bins)
    cut = 12345
    A.fold(be, out, buf, c.off + cut * c.ld, c.rows - cut, c.ld, c.cols, edges, n_bins)
    A.fold(be, out, buf, c.off, cut, c.ld, c.cols, edges, n_bins)
    A.check_case(A.fetch(be, out), c)
    # three views of three cases, one set of outputs (the cases share the 481-bin table)
    parts = [A.case(n) for n in ("3x64", "4097x3_strided", "70000x33_strided")]
    assert all(np.array_equal(p.edges, c.edges) for p in parts)
    out = A.fresh_outputs(be, n_bins)
    for p in parts:
        A.fold(be, out, be.upload(p.buffer), p.off, p.rows, p.ld, p.cols, edges, n_bins)
    got = A.fetch(be, out)
    A.check(got, sum(p.counts for p in parts), sum(p.outside for p in parts), sum(p.finite for p in parts),
            sum(p.nonfinite for p in parts), min(p.lo for p in parts), max(p.hi for p in parts), "three views")
    # a range that starts inside the data is kept where the data does not pass it; an all-NaN view changes no extreme
    out = A.fresh_outputs(be, 1)
    nan = be.upload(np.full(300, np.nan, np.float32))
    be.call("view_range_f32", A.Ref(nan), 3, 100, 100, A.Ref(out["range"]), A.Ref(out["count"]))
    got = A.fetch(be, out)
    assert (got["lo"], got["hi"], got["finite"], got["nonfinite"]) == (float(A.FLT_MAX), -float(A.FLT_MAX), 0, 300)
    small = be.upload(np.asarray([-0.25, -0.0, 0.5], np.float32))
    be.call("view_range_f32", A.Ref(small), 1, 3, 3, A.Ref(out["range"]), A.Ref(out["count"]))
    be.call("view_range_f32", A.Ref(small, 1), 1, 2, 2, A.Ref(out["range"]), A.Ref(out["count"]))
    got = A.fetch(be, out)
    assert (got["lo"], got["hi"], got["finite"], got["nonfinite"]) == (-0.25, 0.5, 5, 300)


def test_accumulation(be):
    check_accumulation(be)


def test_rows_zero_and_views_of_a_pixmap(be):
    c = A.case("5x65_strided")
    out = A.fresh_outputs(be, 1)
    A.fold(be, out, be.upload(c.buffer), c.off, 0, c.ld, c.cols, be.upload(c.edges), 1)
    got = A.fetch(be, out)
    assert (got["lo"], got["hi"], got["finite"], got["counts"].sum()) == (float(A.FLT_MAX), -float(A.FLT_MAX), 0, 0)
    st = SimpleNamespace(pixmap=[4, 5, 6, 9, 11, 12], ch_off=3, ld=40, npix=6)
    assert storage_views(st, 8) == [(4 * 320 + 3, 24), (9 * 320 + 3, 8), (11 * 320 + 3, 16)]
    assert storage_views(SimpleNamespace(pixmap=None, ch_off=7, ld=40, npix=9), 8) == [(7, 72)]


# ----------------------------------------------------------------------------- the bin arithmetic
def test_bins_per_tap():
    sym = lambda npix, c: SimpleNamespace(npix=npix, c=c)  # noqa: E731
    flat = SimpleNamespace(sources=[], features=96)
    taps = [(sym(16, 16), "first"), (sym(4, 32), "half"), (sym(1, 1), "tiny"), (flat, "flat")]
    assert [tap_size(s) for s, _ in taps] == [256, 128, 1, 96]
    assert tap_bins(taps, 480) == {"first": 480, "half": 240, "tiny": 1, "flat": 180}  # int(1.875 * size)
    assert tap_bins(taps[:3], 100) == {"first": 100, "half": 50, "tiny": 1}  # int(0.390625) = 0: clamped to 1
    assert tap_bins([(sym(1, 10), "a"), (sym(1, 85), "b")], 480)["b"] == 4080
    with pytest.raises(ValueError, match="'wide'.*4128"):
        tap_bins([(sym(1, 10), "a"), (sym(1, 86), "wide")], 480)
    assert ACT_MAX_BINS == 4096


# ----------------------------------------------------------------------------- the taps of a tiny HYPELCNN and the tool
def write_checkpoint(tmp, backend):
    """a 12-step run of the tiny HYPELCNN; -> (algorithm parameter file, log directory with its checkpoint)"""
    log_dir = run_episode(tmp, backend, [])
    return str(tmp / "alg.json"), log_dir


def tool_argv(alg_path, log_dir, out_dir, domain, model="HYPELCNNModel"):
    return ["--loader_name", "SyntheticDataLoader", "--path", SCENE, "--neighborhood", "1", "--model_name", model,
            "--algorithm_param_path", alg_path, "--base_log_path", log_dir, "--output_path", str(out_dir),
            "--batch_size", str(BATCH), "--domain", domain]


def host_histograms(run, bins):
    """{tap: (lo, hi, int64 counts summed over the batches)}, number of batches, batch sizes: numpy.histogram on the
    float64 values of every tap fetched from every forward of `run`"""
    fetched, sizes = {name: [] for _, name in run.taps}, []
    for x in run.batches():
        ct = run.forward(x)
        sizes.append(int(x.shape[0]))
        for sym, name in run.taps:
            fetched[name].append(ct.value(sym).cpu().numpy().astype(np.float64).reshape(-1))
    out = {}
    for name, parts in fetched.items():
        lo, hi = min(float(p.min()) for p in parts), max(float(p.max()) for p in parts)
        out[name] = (lo, hi, sum(np.histogram(p, bins=bins[name], range=(lo, hi))[0].astype(np.int64) for p in parts))
    return out, len(sizes), sizes


def check_taps_of_one_forward(backend, alg_path, log_dir):
    flags, _ = tool.build_parser().parse_known_args(tool_argv(alg_path, log_dir, "unused", "sample"))
    run = tool.TapRun(flags, backend)
    assert [name for _, name in run.taps] == TAPS
    bins = tap_bins(run.taps, 480)
    acts = ActivationTaps(run.session, run.taps, bins)
    x = next(run.batches())
    ct = run.forward(x)
    acts.fold_range(ct)
    edges = acts.set_edges()
    acts.fold_histogram(ct)
    got = acts.results()
    for sym, name in run.taps:
        value = ct.value(sym).cpu().numpy().astype(np.float64)
        r = got[name]
        assert value.size == tap_size(sym) * BATCH and np.isfinite(value).all()
        assert (r["lo"], r["hi"]) == (float(value.min()), float(value.max())), name
        want, made = np.histogram(value, bins=bins[name], range=(r["lo"], r["hi"]))
        assert np.array_equal(made, edges[name]) and np.array_equal(r["edges"], made), name
        assert np.array_equal(r["counts"], want), (name, np.flatnonzero(r["counts"] != want)[:8])
        assert r["outside"] == 0 and r["nonfinite"] == 0 and int(r["counts"].sum()) == r["finite"] == value.size, name


def check_tool(backend, alg_path, log_dir, out_dir, domain, capsys):
    argv = tool_argv(alg_path, log_dir, out_dir, domain)
    records = tool.main(argv, backend=backend)
    assert capsys.readouterr().out.rstrip().splitlines()[-1].startswith("Done evaluation(")
    flags, _ = tool.build_parser().parse_known_args(argv)
    run = tool.TapRun(flags, backend)  # a second session restored from the same checkpoint
    bins = tap_bins(run.taps, 480)
    want, n_batches, sizes = host_histograms(run, bins)
    if domain == "controlled":
        assert sizes == [BATCH]
    else:
        assert len(sizes) > 2 and sizes[-1] not in (0, BATCH) and set(sizes[:-1]) == {BATCH}  # a partial last batch
    try:
        import matplotlib  # noqa: F401
        plots = True
    except ImportError:
        plots = False
    assert sorted(records) == sorted(TAPS)
    for sym, name in run.taps:
        with open(os.path.join(str(out_dir), name + "_hist.json")) as f:
            rec = json.load(f)
        assert rec == records[name] and sorted(rec) == sorted(
            ["name", "bins", "lo", "hi", "counts", "mean", "batches", "finite", "nonfinite", "outside"])
        lo, hi, counts = want[name]
        assert (rec["name"], rec["bins"], rec["batches"]) == (name, bins[name], n_batches)
        assert (rec["lo"], rec["hi"]) == (lo, hi), name
        assert rec["counts"] == counts.tolist(), name
        assert rec["mean"] == (counts / n_batches).tolist()
        assert rec["finite"] == sum(sizes) * tap_size(sym) == sum(rec["counts"])
        assert rec["nonfinite"] == 0 and rec["outside"] == 0
        assert os.path.exists(os.path.join(str(out_dir), name + "_fig.jpg")) == plots
    return records


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    return write_checkpoint(tmp_path_factory.mktemp("activation"), EmuBackend())


def test_taps_of_one_forward(be, checkpoint):
    check_taps_of_one_forward(be, *checkpoint)


@pytest.mark.parametrize("domain", ["controlled", "sample"])
def test_tool_end_to_end(be, checkpoint, tmp_path, capsys, domain):
    records = check_tool(be, *checkpoint, tmp_path / "out", domain, capsys)
    if domain == "controlled":  # identical samples: every count is a multiple of the batch size
        assert all(c % BATCH == 0 for r in records.values() for c in r["counts"])


def test_a_model_without_taps_is_refused_by_name(be, checkpoint, tmp_path):
    alg = tmp_path / "dual.json"
    alg.write_text(json.dumps(dict(ALG, hs_lidar_diff=1)))
    with pytest.raises(ValueError, match="DUALCNNModel"):
        tool.main(tool_argv(str(alg), checkpoint[1], tmp_path, "controlled", model="DUALCNNModel"), backend=be)


def test_too_many_bins_are_refused_by_tap_name(be, checkpoint, tmp_path):
    with pytest.raises(ValueError, match="spectral_expansion|spectral_reduction|spatial|classification"):
        tool.main(tool_argv(*checkpoint, tmp_path, "controlled") + ["--base_bins", "100000"], backend=be)


# ----------------------------------------------------------------------------- the reference's model through the facade
@pytest.mark.skipif(not os.path.isdir("/root/reference/nnmodel"), reason="needs the reference checkout")
def test_the_facade_carries_the_reference_taps():
    from hypelcnn_amd import graph as G, tf_facade
    from hypelcnn_amd.common import common_nn_ops as P

    def taps_of(model):
        tower = G.Tower(G.VariableStore("nn_core"), False)
        x = tower.placeholder("x", (3, 3), 11)
        out = model.create_tensor_graph(P.ModelInputParams(x=x, y=None, device_id="/gpu:0", is_training=False), 3,
                                        dict(ALG))
        return [(pair.name, pair.tensor.get_shape()) for pair in out.histogram_tensors]

    native = taps_of(P.get_model_from_name("HYPELCNNModel"))
    assert [n for n, _ in native] == TAPS
    assert taps_of(tf_facade.reference_model("HYPELCNNModel", "/root/reference")) == native
