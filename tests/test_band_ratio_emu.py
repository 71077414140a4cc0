"""CPU: the band-ratio statistics on the NumPy twins of their two launches (tests/emu_band_ratio.py) -- the host layer
against numpy.percentile, the opt-in wiring of gan_infer_for_shadow, and measure_targets_shadow_ratio on a host and a
device-resident scene."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import tests.emu_band_ratio  # noqa: F401 -- registers the band-ratio launches on EmuBackend
import tests.emu_pairs  # noqa: F401 -- and the pairing launches of a device-resident scene
import tests.emu_scene  # noqa: F401
from hypelcnn_amd.backend import Ref
from hypelcnn_amd.common import band_ratio as BR
from hypelcnn_amd.gan import gan_infer_for_shadow as GS
from hypelcnn_amd.gan.wrapper_registry import get_infer_wrapper_dict, get_sampling_map
from hypelcnn_amd.gan.wrappers import gan_common as C
from hypelcnn_amd.loader.SyntheticDataLoader import SyntheticDataLoader
from hypelcnn_amd.utilities import measure_targets_shadow_ratio as MT
from tests import band_ratio_cases as K
from tests.emu_backend import EmuBackend
from tests.test_gan_inference import SCENE, DenormEmu, _trained_checkpoint

QS = (10, 50, 90)


def numpy_stats(ratio):
    """The statistics from a float32 ratio matrix, NumPy only: the rule band_ratio_stats documents."""
    kept = ratio[np.isfinite(ratio).all(axis=1)].astype(np.float64)
    out = {"samples": ratio.shape[0], "kept": kept.shape[0]}
    if kept.shape[0] == 0:
        return out
    for q in QS:
        out[f"p{q}"] = np.percentile(kept, q, axis=0)
    out["mean"], out["std"] = kept.mean(axis=0), kept.std(axis=0)
    return out


def check_stats(got, want):
    assert got["samples"] == want["samples"] and got["kept"] == want["kept"]
    for q in QS:
        g, w = np.asarray(got[f"p{q}"], np.float64), want[f"p{q}"]
        assert g.shape == w.shape and np.array_equal(g, w), (q, np.abs(g - w).max())  # bit for bit (0.0 == -0.0)
    # float64 sums of at most 10^4 float32 terms: the two summation orders differ by a few 1e-16 relative per term
    np.testing.assert_allclose(got["mean"], want["mean"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["std"], want["std"], rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("case", K.stats_cases(), ids=lambda c: c[0])
def test_stats_are_numpys_percentiles_of_the_float64_ratios(case):
    _, num, den, scale = case
    ratio, _ = K.expected_ratio(num, den, scale, num.shape[1])
    be = EmuBackend()
    got = BR.band_ratio_stats(be, num, den, scale)
    check_stats(got, numpy_stats(ratio))
    assert be.launch_log == ["band_ratio_f32", "column_rank_select_f32"]  # one select for all ranks


def test_row_strided_views_are_read_in_place():
    num, den, scale = K.ratio_case(65, 7, 3)
    ratio, _ = K.expected_ratio(num, den, scale, 7)
    got = BR.band_ratio_stats(EmuBackend(), torch.from_numpy(num)[:, :7], torch.from_numpy(den)[:, :7],
                              torch.from_numpy(scale))
    check_stats(got, numpy_stats(ratio))
    ref, ld, n, bands = BR._rows(EmuBackend(), torch.from_numpy(num)[:, :7])
    assert (ld, n, bands) == (10, 65, 7) and ref.t.data_ptr() == num.ctypes.data  # no copy


def test_more_percentiles_than_one_select_holds():
    rng = np.random.default_rng(4)
    num, den = rng.random((501, 6)).astype(np.float32), (rng.random((501, 6)) + 0.5).astype(np.float32)
    qs = (1, 5, 10, 25, 50, 75, 99.5)
    be = EmuBackend()
    got = BR.band_ratio_stats(be, num, den, None, percentiles=qs)
    assert be.launch_log == ["band_ratio_f32"] + ["column_rank_select_f32"] * 2
    for q in qs:
        assert np.array_equal(got[f"p{q:g}"], np.percentile((num / den).astype(np.float64), q, axis=0))


def test_no_kept_row_gives_nan_and_launches_no_select(tmp_path):
    num = np.ones((9, 4), np.float32)
    den = np.ones((9, 4), np.float32)
    den[:, 2] = 0
    be = EmuBackend()
    got = BR.band_ratio_stats(be, num, den, None)
    assert got["samples"] == 9 and got["kept"] == 0 and be.launch_log == ["band_ratio_f32"]
    for key in ("p10", "p50", "p90", "mean", "std"):
        assert got[key].shape == (4,) and np.isnan(got[key]).all()
    record = BR.write_band_ratio(str(tmp_path), "band_ratio_x", 7, np.arange(4.0), got, "p50", "p10", "p90")
    assert os.listdir(tmp_path) == ["band_ratio_x_7.json"]  # numbers always, no figure
    assert json.load(open(tmp_path / "band_ratio_x_7.json")) == record and record["p50"] == [None] * 4


def test_twin_of_the_select_on_the_shared_cases():
    """The rank-select twin against a per-column Python sort on a few of the device cases (ranks unsorted, repeated)."""
    be = EmuBackend()
    for kind in K.DATA_SETS:
        n, bands, m, pad = 65, 7, 64, 2
        x, ok = K.select_case(kind, n, bands, m, pad)
        ranks = K.ranks_for(m, 6)
        out = torch.zeros(6 * bands)
        ws = be.empty(bands * 2320, torch.int32)
        be.call("column_rank_select_f32", Ref(torch.from_numpy(x.reshape(-1))), bands + pad, n, bands,
                Ref(torch.from_numpy(ok)), m, Ref(torch.tensor(ranks)), 6, Ref(out), Ref(ws))
        got = out.numpy().reshape(6, bands)
        for b in range(bands):
            col = sorted(float(v) for v in x[ok != 0, b])
            assert [float(v) for v in got[:, b]] == [col[r] for r in ranks], (kind, b)


def test_figure_is_a_pdf_and_leaves_no_global_state(tmp_path):
    pytest.importorskip("matplotlib")
    import matplotlib
    before = dict(matplotlib.rcParams)
    bands = np.linspace(400, 1000, 16)
    path = BR.plot_band_ratio(bands, np.full(16, 0.5), np.full(16, 0.3), np.full(16, 0.8), 12, "band_ratio_t",
                              str(tmp_path))
    assert path == str(tmp_path / "band_ratio_t_12.pdf") and open(path, "rb").read(4) == b"%PDF"
    assert dict(matplotlib.rcParams) == before
    import sys
    assert "matplotlib.pyplot" not in sys.modules or not sys.modules["matplotlib.pyplot"].get_fignums()


# ----------------------------------------------------------------------------- gan_infer_for_shadow, opt-in
def _have_matplotlib():
    try:
        import matplotlib.figure  # noqa: F401
        return True
    except ImportError:
        return False


def test_infer_cli_writes_the_band_ratio_only_when_asked(tmp_path):
    ckpt = _trained_checkpoint(tmp_path, "cycle_gan", steps=3)
    runs = {}
    for name, extra in (("off", []), ("on", ["--band_ratio_stats", "true"])):
        base = str(tmp_path / name / "model.ckpt-3.npz")
        os.makedirs(os.path.dirname(base))
        shutil.copy(ckpt, base)
        divs = GS.main(["--loader_name", "SyntheticDataLoader", "--path", SCENE, "--base_log_path", base,
                        "--number_of_samples", "200", "--gan_type", "cycle_gan"] + extra, backend=DenormEmu())
        runs[name] = (divs, base[:-4])
    today = ["best_ratio_deshadowed.json", "best_ratio_shadowed.json", "summaries.jsonl"]
    assert sorted(os.listdir(runs["off"][1])) == today
    added = [f"band_ratio_{s}_0.{e}" for s in ("shadowed", "deshadowed")
             for e in (("json", "pdf") if _have_matplotlib() else ("json",))]
    assert sorted(os.listdir(runs["on"][1])) == sorted(today + added)
    assert runs["on"][0] == runs["off"][0] and len(runs["on"][0]) == 2  # the divergences do not move

    # the numbers, recomputed in NumPy from the hook's own samples and its generator's output
    loader = SyntheticDataLoader(SCENE)
    ds = loader.load_data(0, True)
    smap, shadow_ratio = loader.load_shadow_map(0, ds)
    wrapper = get_infer_wrapper_dict()["cycle_gan"]
    from hypelcnn_amd.gan.gan_utilities import load_gan_variables
    peer = wrapper.create_inference_hook(ds, loader, str(tmp_path / "again"), 0, smap, shadow_ratio, 0, 200,
                                         backend=DenormEmu())
    os.makedirs(tmp_path / "again")
    sess = C.restore_generators(peer.ctx, wrapper.create_generator_restorer(), load_gan_variables(ckpt))
    assert peer.band_ratio_stats is False
    for hook in peer._validation_base_hooks:
        x = hook._data_sample_list
        ct = sess.compile_phase(peer.ctx.tower, x.shape[0], outputs=[hook._infer_model], key="check" + hook._name_suffix)
        ct.set_input(hook._input_tensor.name, torch.as_tensor(x))
        ct.forward()
        gen = ct.value(hook._infer_model, copy=True).numpy()
        assert gen.dtype == np.float32 and gen.shape == x.shape
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = gen / x * np.asarray(hook._shadow_ratio, np.float32)
        want = numpy_stats(ratio)
        got = json.load(open(os.path.join(runs["on"][1], f"band_ratio_{hook._name_suffix}_0.json")))
        assert got["step"] == 0 and got["bands"] == [float(v) for v in loader.get_band_measurements()]
        assert want["kept"] > 0
        check_stats({k: (np.asarray(v, np.float64) if isinstance(v, list) else v) for k, v in got.items()}, want)
        if _have_matplotlib():
            with open(os.path.join(runs["on"][1], f"band_ratio_{hook._name_suffix}_0.pdf"), "rb") as f:
                assert f.read(4) == b"%PDF"


def test_peer_hook_passes_the_switch_to_its_members():
    class Member:
        band_ratio_stats = False

    a, b = Member(), Member()
    peer = C.PeerValidationHook(a, b)
    assert peer.band_ratio_stats is False
    peer.band_ratio_stats = True
    assert a.band_ratio_stats is True and b.band_ratio_stats is True and peer.band_ratio_stats is True


# ----------------------------------------------------------------------------- measure_targets_shadow_ratio
@pytest.mark.parametrize("pairing", ["random", "neighbour", "target", "dummy"])
def test_measure_targets_on_a_host_and_a_device_scene(tmp_path, pairing):
    scene = "grss2013:h=30:w=40"
    results = {}
    for where, path in (("host", scene), ("device", scene + ":device=1")):
        out = tmp_path / where
        results[where] = MT.main(["--loader_name", "SyntheticDataLoader", "--path", path, "--pairing_method", pairing,
                                  "--output_path", str(out)], backend=EmuBackend())
        names = [f"syntheticdataloader_{pairing}_0.json"] + \
            ([f"syntheticdataloader_{pairing}_0.pdf"] if _have_matplotlib() else [])
        assert sorted(os.listdir(out)) == names
    host, device = results["host"], results["device"]
    assert host.keys() == device.keys()
    for key in host:
        assert np.array_equal(np.asarray(host[key]), np.asarray(device[key])), key
    loader = SyntheticDataLoader(scene)
    ds = loader.load_data(0, True)
    smap, _ = loader.load_shadow_map(0, ds)
    normal, shadow = get_sampling_map()[pairing].get_sample_pairs(ds, loader, smap)
    bands = ds.get_casi_band_count()
    normal = np.asarray(normal, np.float32).reshape(normal.shape[0], -1)[:, :bands]
    shadow = np.asarray(shadow, np.float32).reshape(shadow.shape[0], -1)[:, :bands]
    with np.errstate(divide="ignore", invalid="ignore"):
        want = numpy_stats(shadow / normal)
    assert want["kept"] > 0
    check_stats(host, want)
    record = json.load(open(tmp_path / "host" / f"syntheticdataloader_{pairing}_0.json"))
    assert record["step"] == 0 and record["kept"] == want["kept"] and record["mean"] == [float(v) for v in host["mean"]]
    assert record["bands"] == [float(v) for v in loader.get_band_measurements()]


# ----------------------------------------------------------------------------- gan_train_for_shadow, opt-in
def test_train_cli_writes_the_band_ratio_of_its_closing_statistic_when_asked(tmp_path):
    from tests.test_training_loop_emu import _gan_params
    GT, params = _gan_params(tmp_path, "cycle_gan", 2, SCENE, 16)
    assert GT.build_parser().parse_known_args([])[0].band_ratio_stats is False
    assert GT.build_parser().parse_known_args(["--band_ratio_stats", "true"])[0].band_ratio_stats is True
    params["path"] = SCENE
    logs = {}
    for name, on in (("off", False), ("on", True)):
        run = dict(params, base_log_path=str(tmp_path / name / "gan"), band_ratio_stats=on)
        divs = GT.run_session(run, run["base_log_path"], backend=DenormEmu())
        logs[name] = (divs, f"{run['base_log_path']}_{GT.get_log_suffix(type('F', (), run))}")
    assert logs["on"][0] == logs["off"][0]
    assert all(f.startswith("model.ckpt-") for f in os.listdir(logs["off"][1]))  # nothing new by default
    extra = sorted(f for f in os.listdir(logs["on"][1]) if not f.startswith("model.ckpt-"))
    assert extra == ["band_ratio_shadowed_2.json"] + (["band_ratio_shadowed_2.pdf"] if _have_matplotlib() else [])
    record = json.load(open(os.path.join(logs["on"][1], "band_ratio_shadowed_2.json")))
    assert record["step"] == 2 and 0 < record["kept"] <= record["samples"] and len(record["p50"]) == 16
    assert all(a <= b <= c for a, b, c in zip(record["p10"], record["p50"], record["p90"]))


def test_moments_are_taken_a_block_of_rows_at_a_time():
    rng = np.random.default_rng(6)
    ratio = (rng.standard_normal((1001, 7)) * 3 + 1).astype(np.float32)
    keep = rng.random(1001) < 0.8
    keep[64:128] = False  # a block without a kept row
    want = ratio[keep].astype(np.float64)
    for chunk in (7 * 64, 7 * 1001, 1 << 22, 1):
        mean, std = BR._moments(torch.from_numpy(ratio), torch.from_numpy(keep), int(keep.sum()), chunk_elements=chunk)
        np.testing.assert_allclose(mean, want.mean(axis=0), rtol=1e-9, atol=0)
        np.testing.assert_allclose(std, want.std(axis=0), rtol=1e-9, atol=0)
