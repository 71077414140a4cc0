"""CPU (numpy kernel emulation): --tensorboard_events end to end -- a short SyntheticDataLoader run writes an event file
next to summaries.jsonl, utilities/read_summary_file pulls the validation confusion matrices out of it and
utilities/stat_extractor turns them into OA / AA / kappa; the --log_model_params histograms come from the summary
launch (here its twin, tests/emu_summary.py).  Without the flag the log directory holds no event file."""
import glob
import json
import os

import numpy as np
import pytest

import tests.emu_summary as E
from hypelcnn_amd.classify import train_for_classification as T
from hypelcnn_amd.common import tb_events
from hypelcnn_amd.common.common_nn_ops import confusion_metrics
from hypelcnn_amd.utilities import read_summary_file, stat_extractor
from tests import summary_cases as C
from tests.emu_backend import EmuBackend

ALG = {"batch_size": 32, "drop_out_ratio": 0.3, "filter_count": 32, "learning_rate": 3e-3,
       "learning_rate_decay_factor": 0.96, "learning_rate_decay_step": 350, "lrelu_alpha": 0.18,
       "optimizer": "AdamOptimizer", "bn_decay": 0.9, "l2regularizer_scale": 1e-5, "spectral_hierarchy_level": 1,
       "spatial_hierarchy_level": 1, "degradation_coeff": 3, "use_residual": True}
SCALARS = ("training_cross_entropy", "training_learning_rate", "test_overall_accuracy", "validation_overall_accuracy",
           "validation_average_accuracy", "validation_kappa")


def run_episode(tmp_path, backend, extra, steps=12):
    p = tmp_path / "alg.json"
    p.write_text(json.dumps(ALG))
    argv = ["--loader_name", "SyntheticDataLoader", "--path", "grss2013:h=24:w=30:bands=10:classes=3:samples=0.6",
            "--neighborhood", "1", "--model_name", "HYPELCNNModel", "--algorithm_param_path", str(p),
            "--batch_size", "32", "--step", str(steps), "--base_log_path", str(tmp_path / "log"),
            "--perform_validation", "true", "--validation_steps", "5", "--save_checkpoint_steps", "50"] + list(extra)
    flags, _ = T.build_parser().parse_known_args(argv)
    log_dir = os.path.join(flags.base_log_path, T.get_log_suffix(flags))
    T.perform_an_episode(flags, dict(ALG), T.get_model_from_name(flags.model_name), log_dir, backend=backend)
    return log_dir


def check_events_of_run(log_dir, tmp_path, monkeypatch, capsys):
    """what both the emulated and the device run must satisfy; -> {step: {tag: histogram}}"""
    files = glob.glob(os.path.join(log_dir, "events.out.tfevents.*"))
    assert len(files) == 1
    events = list(tb_events.read_events(files[0]))
    assert events[0]["file_version"] == "brain.Event:2" and not events[0]["values"]
    start = events[1]
    assert start["step"] == 0 and [v["tag"] for v in start["values"]] == ["flags", "algorithm_params"]
    for v in start["values"]:
        text = v["tensor"]["string_val"][0].decode()
        assert v["plugin_name"] == "text" and v["tensor"]["shape"] == [] and v["tensor"]["dtype"] == 7
        assert text.startswith("<pre>{") and text.endswith("}</pre>")
    records = [json.loads(line) for line in open(os.path.join(log_dir, "summaries.jsonl"))]
    assert "flags" in records[0] and "histograms" not in records[0]
    assert [e["step"] for e in events[2:]] == [r["step"] for r in records[1:]] and len(records) >= 3
    with np.load(glob.glob(os.path.join(log_dir, "model.ckpt-*.npz"))[-1]) as z:
        saved = {k.replace("|", "/"): z[k].size for k in z.files if k.startswith("nn_core")}
    assert saved
    histograms, confusions = {}, {}
    for rec, ev in zip(records[1:], events[2:]):
        assert "histograms" not in rec
        by_tag = {v["tag"]: v for v in ev["values"]}
        for tag in SCALARS:
            assert (tag in rec) == (tag in by_tag)
            if tag in rec:
                assert by_tag[tag]["simple_value"] == float(np.float32(rec[tag])), tag
        for tag in ("test_confusion", "validation_confusion"):
            assert (tag in rec) == (tag in by_tag)
            if tag in rec:
                t, m = by_tag[tag]["tensor"], np.asarray(rec[tag])
                assert t["dtype"] == 7 and t["shape"] == list(m.shape) and by_tag[tag]["plugin_name"] == "text"
                assert [s.decode() for s in t["string_val"]] == [str(x) for x in m.reshape(-1)]
        if "validation_confusion" in rec:
            confusions[rec["step"]] = np.asarray(rec["validation_confusion"])
        histo = {t: v["histo"] for t, v in by_tag.items() if "histo" in v}
        assert set(histo) == set(saved) == set(rec["variable_norms"])  # the checkpoint's nn_core/* names
        for name, h in histo.items():
            assert h["num"] == saved[name] and sum(h["bucket"]) == saved[name], name
            assert abs(rec["variable_norms"][name] - np.sqrt(h["sum_squares"])) <= 1e-12 * (1 + rec["variable_norms"][name])
        histograms[rec["step"]] = histo
    assert confusions
    # the reference's tool chain: event file -> CSVs -> OA / AA / kappa
    monkeypatch.chdir(tmp_path)
    found = read_summary_file.main([log_dir])
    assert sorted(s for s, _, _ in found) == sorted(confusions)
    parent = os.path.basename(log_dir)
    for step, path, _ in found:
        assert path == os.path.join(".", f"log_{parent}_s{step}.csv")
        assert np.array_equal(np.loadtxt(path, dtype=int, delimiter=",", ndmin=2), confusions[step])
    only = sorted(confusions)[-1]
    assert [s for s, _, _ in read_summary_file.main([log_dir, str(only)])] == [only]
    csv_dir = tmp_path / "one"
    csv_dir.mkdir()
    os.replace(f"log_{parent}_s{only}.csv", csv_dir / "m.csv")
    holder = stat_extractor.extract_statistics_info(stat_extractor.get_conf_list_from_directory(str(csv_dir)))
    oa, aa, kappa = confusion_metrics(confusions[only])
    assert abs(holder.oa_array[0] - oa) <= 1e-12 and abs(holder.kappa_array[0] - kappa) <= 1e-12
    assert abs(np.mean(holder.aa_array[0]) - aa) <= 1e-12
    stat_extractor.main([str(csv_dir)])
    assert "OA: %.4f AA: %.4f Kappa: %.4f" % (oa, aa, kappa) in capsys.readouterr().out
    return histograms


def test_events_end_to_end_on_the_emulation(tmp_path, monkeypatch, capsys):
    be = EmuBackend()
    log_dir = run_episode(tmp_path, be, ["--tensorboard_events", "true", "--log_model_params", "true"])
    histograms = check_events_of_run(log_dir, tmp_path, monkeypatch, capsys)
    # the last record is taken at the step the final checkpoint saves: its histograms are those of the saved variables
    last = max(histograms)
    with np.load(os.path.join(log_dir, f"model.ckpt-{last}.npz")) as z:
        for name, h in histograms[last].items():
            stats, bad, counts = E.summarize(z[name.replace("/", "|")], C.LIMITS)
            lim, cnt = tb_events.collapse_buckets(C.LIMITS, counts)
            assert bad == 0 and (h["min"], h["max"], h["num"]) == stats[:3], name
            assert h["bucket_limit"] == lim and h["bucket"] == cnt, name


def test_events_without_histograms(tmp_path):
    log_dir = run_episode(tmp_path, EmuBackend(), ["--tensorboard_events"], steps=3)
    (path,) = glob.glob(os.path.join(log_dir, "events.out.tfevents.*"))
    events = list(tb_events.read_events(path))
    assert len(events) >= 3 and not any("histo" in v for e in events for v in e["values"])
    assert not any("variable_norms" in json.loads(line) for line in open(os.path.join(log_dir, "summaries.jsonl")))


def test_flag_off_writes_no_event_file(tmp_path):
    log_dir = run_episode(tmp_path, EmuBackend(), ["--log_model_params", "true"], steps=3)
    assert not [f for f in os.listdir(log_dir) if f.startswith("events")]
    records = [json.loads(line) for line in open(os.path.join(log_dir, "summaries.jsonl"))]
    assert any("variable_norms" in r for r in records)


def test_non_finite_variable_gets_a_line_instead_of_a_histogram(capsys):
    from hypelcnn_amd.classify.monitored_session_runner import record_to_summary_values
    counts = np.zeros(C.LIMITS.size, np.int64)
    counts[800] = 3
    good = {"min": 1.0, "max": 2.0, "num": 3.0, "sum": 4.0, "sum_squares": 6.0, "nonfinite": 0, "buckets": counts}
    values = record_to_summary_values({"step": 4, "training_cross_entropy": 0.5},
                                      (C.LIMITS, {"nn_core/a": good, "nn_core/b": dict(good, nonfinite=2)}))
    ev = tb_events.decode_event(tb_events.encode_event(1.0, 4, values))
    assert [v["tag"] for v in ev["values"]] == ["training_cross_entropy", "nn_core/a"]
    assert "nn_core/b" in capsys.readouterr().out


# ----------------------------------------------------------------------------- the launch itself, on the twin
def test_launch_contract_on_the_emulation():
    be = EmuBackend()
    buf, segments, tensors = C.layout([C.boundary_values(), np.zeros(0, np.float32),
                                       np.asarray([np.nan, 1.0, np.inf, -np.inf, -2.0], np.float32)], order=[2, 0, 1])
    got = C.launch(be, buf, segments)
    C.check_against_twin(got, tensors)
    stats, nonfinite, buckets = got
    assert nonfinite.tolist() == [3, 0, 0] and stats[0].tolist() == [-2.0, 1.0, 2.0, -1.0, 5.0]
    assert stats[2].tolist()[:3] == [E.DBL_MAX, -E.DBL_MAX, 0.0] and buckets[2].sum() == 0
    # [0, 1e-12): +-0, the two positive subnormals, FLT_MIN and the float32 just below 1e-12
    assert buckets[1][776] == 6 and buckets[1].sum() == tensors[1].size
    assert buckets.sum() == sum(np.isfinite(t).sum() for t in tensors)  # the sentinel gaps are not counted


def test_slice_count_mismatch_is_refused():
    from hypelcnn_amd.common.device_summary import TensorSummary
    be = EmuBackend()
    ts = TensorSummary(be, be.upload(np.ones(100, np.float32)), [(0, 50), (50, 50)], be.upload(C.LIMITS), C.LIMITS.size)
    ts.slices += 1
    ts.ws = be.zeros(ts.n + 1 + 6 * ts.slices, ts.ws.dtype)
    ts.launch()
    with pytest.raises(RuntimeError):
        ts.results()
