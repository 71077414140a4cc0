"""CPU (numpy kernel emulation): --flag_config_file_opt through both trainers, and the GAN trainer's peer validation
hook on the training session (--validate_while_training)."""
import json
import math
import os

import pytest

import tests.emu_band_ratio  # noqa: F401 -- registers the band-ratio launches on EmuBackend
import tests.emu_pairs  # noqa: F401 -- and the pairing launches of a device-resident scene
import tests.emu_scene  # noqa: F401
from hypelcnn_amd.classify import train_for_classification as T
from hypelcnn_amd.common import hyperopt as H
from hypelcnn_amd.gan import gan_train_for_shadow as GT
from tests.emu_backend import EmuBackend
from tests.test_gan_inference import DenormEmu

OPT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "opt")
CLS_SCENE = "grss2013:h=24:w=30:bands=10:classes=3:samples=0.6"  # the scene of tests/test_training_loop_emu._flags
GAN_SCENE = "avon:h=40:w=60:bands=16"
CUT_SCENE = "avon:h=40:w=60:bands=24"  # the patch-NCE models need the wider spectrum (tests/test_training_loop_emu.py)


def classifier_argv(tmp_path, steps, trials, runs, space=None, validation=True):
    """The flags of tests/test_training_loop_emu._flags, as a command line, plus the study's."""
    return ["--loader_name", "SyntheticDataLoader", "--path", CLS_SCENE, "--neighborhood", "1", "--model_name",
            "HYPELCNNModel", "--batch_size", "32", "--step", str(steps), "--base_log_path", str(tmp_path / "log"),
            "--validation_steps", "60", "--save_checkpoint_steps", "50", "--unknown_flag_is_ignored", "1",
            "--flag_config_file_opt", space or os.path.join(OPT_DIR, "classification_opt_small.json"),
            "--opt_trial_count", str(trials), "--opt_run_count", str(runs), "--opt_seed", "0",
            "--opt_storage", str(tmp_path / "study.db")] + (["--perform_validation", "true"] if validation else [])


# ----------------------------------------------------------------------------- 5. classifier
def test_classifier_study(tmp_path, capsys):
    study = T.main(classifier_argv(tmp_path, 6, 3, 2), backend=EmuBackend())
    out = capsys.readouterr().out
    assert isinstance(study, H.Study) and study.study_name == "classification_opt"
    trials = study.trials
    assert [t.state for t in trials] == [H.COMPLETE] * 3 and all(0.0 <= t.value <= 1.0 for t in trials)
    for t in trials:
        assert t.params.keys() == {"drop_out_ratio", "filter_count", "learning_rate"}
        assert 0.001 <= t.params["learning_rate"] <= 0.01 and t.params["filter_count"] in (16, 32)
    dirs = [d for d in os.listdir(tmp_path) if d.startswith("log_")]
    assert len(set(dirs)) == 6 and all(len(d) == len("log_") + 5 for d in dirs), dirs
    assert all(any(f.startswith("model.ckpt-") for f in os.listdir(tmp_path / d)) for d in dirs)
    assert "Running in hyper parameter optimization mode" in out
    assert out.count("Starting run#") == 6 and "Trial 2 finished with value:" in out
    assert os.path.exists(tmp_path / "study.db")


def test_classifier_study_needs_a_validation_result(tmp_path, monkeypatch):
    monkeypatch.setattr(T, "perform_an_episode", lambda *a, **k: pytest.fail("an episode ran"))
    with pytest.raises(ValueError, match="--perform_validation"):
        T.main(classifier_argv(tmp_path, 6, 3, 2, validation=False), backend=EmuBackend())
    assert not os.path.exists(tmp_path / "study.db")


def test_classifier_study_is_refused_under_data_parallelism(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(T, "perform_an_episode", lambda *a, **k: pytest.fail("an episode ran"))
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        T.main(classifier_argv(tmp_path, 6, 3, 2), backend=EmuBackend())


# ----------------------------------------------------------------------------- 6. GAN: validation while training
def gan_params(tmp_path, gan_type, extra=(), scene=GAN_SCENE):
    flags, _ = GT.build_parser().parse_known_args(
        ["--loader_name", "SyntheticDataLoader", "--path", scene, "--gan_type", gan_type, "--batch_size", "16",
         "--step", "6", "--base_log_path", str(tmp_path / "gan"), "--validation_steps", "2",
         "--validation_sample_count", "64"] + list(extra))
    return dict(vars(flags))


def log_dir_of(params):
    return f"{params['base_log_path']}_{GT.get_log_suffix(type('F', (), params))}"


def run_with_hook(params, backend, monkeypatch):
    """run_session, keeping the hook it installs."""
    hooks = []
    real = GT._peer_validation_hook
    monkeypatch.setattr(GT, "_peer_validation_hook", lambda *a, **k: (hooks.append(real(*a, **k)), hooks[-1])[1])
    result = GT.run_session(params, params["base_log_path"], backend=backend)
    monkeypatch.setattr(GT, "_peer_validation_hook", real)
    return result, hooks


def summary_steps(log_dir):
    lines = [json.loads(l) for l in open(os.path.join(log_dir, "summaries.jsonl"))]
    out = {}
    for rec in lines:
        (key,) = [k for k in rec if k.startswith("divergence_")]
        out.setdefault(key, []).append(rec["step"])
        assert math.isfinite(rec[key])
    return out


def check_validated_session(result, hooks, log_dir, suffixes):
    (hook,) = hooks
    base = hook._validation_base_hooks if hasattr(hook, "_validation_base_hooks") else [hook]
    assert len(base) == len(suffixes)
    extra = sorted(f for f in os.listdir(log_dir) if not f.startswith("model.ckpt-"))
    assert extra == sorted([f"best_ratio_{s}.json" for s in suffixes] + ["summaries.jsonl"])
    assert summary_steps(log_dir) == {f"divergence_{s}": [2, 4, 6] for s in suffixes}
    uppers = [h.get_best_upper_div() for h in base]
    means = [h.get_best_mean_div() for h in base]
    assert result == [max(uppers), max(means)] and all(math.isfinite(v) for v in result)
    for h, s in zip(base, suffixes):
        stored = json.load(open(os.path.join(log_dir, f"best_ratio_{s}.json")))
        assert sorted(step for step, _ in stored) == [2, 4, 6]
        assert stored[0][1] == h.get_best_mean_div() == min(v for _, v in stored)
    assert sorted(f for f in os.listdir(log_dir) if f.startswith("model.ckpt-")) == \
        ["model.ckpt-2.npz", "model.ckpt-4.npz", "model.ckpt-6.npz"]


def test_gan_validates_while_it_trains(tmp_path, monkeypatch):
    on = gan_params(tmp_path / "on", "cycle_gan", ["--validate_while_training"])
    assert on["validate_while_training"] is True
    result, hooks = run_with_hook(on, DenormEmu(), monkeypatch)
    check_validated_session(result, hooks, log_dir_of(on), ["shadowed", "deshadowed"])
    # without the flag: checkpoints only, and the closing statistic -- whatever it is, it is what the same call gives
    # with the hook code out of the way
    off = gan_params(tmp_path / "off", "cycle_gan")
    assert off["validate_while_training"] is False
    result_off, hooks_off = run_with_hook(off, DenormEmu(), monkeypatch)
    assert hooks_off == [] and len(result_off) == 2 and all(math.isfinite(v) for v in result_off)
    assert all(f.startswith("model.ckpt-") for f in os.listdir(log_dir_of(off)))
    del off["validate_while_training"]  # a params dict from before the flag existed
    off["base_log_path"] = str(tmp_path / "off2" / "gan")
    assert GT.run_session(off, off["base_log_path"], backend=DenormEmu()) == result_off


@pytest.mark.parametrize("gan_type, suffix", [("gan_x2y", "shadowed"), ("gan_y2x", "deshadowed"), ("cut_x2y", "shadowed"),
                                              ("dcl_gan", None)])
def test_one_generator_wrappers_install_one_hook(tmp_path, monkeypatch, gan_type, suffix):
    """The reference has no `--gan_type gan`: its one-generator types are gan_x2y / gan_y2x (and the CUT pair)."""
    params = gan_params(tmp_path, gan_type, ["--validate_while_training", "true"],
                        scene=GAN_SCENE if gan_type.startswith("gan") else CUT_SCENE)
    result, hooks = run_with_hook(params, DenormEmu(), monkeypatch)
    check_validated_session(result, hooks, log_dir_of(params), [suffix] if suffix else ["shadowed", "deshadowed"])


def test_band_ratio_stats_go_through_the_hook(tmp_path, monkeypatch):
    params = gan_params(tmp_path, "gan_x2y", ["--validate_while_training", "--band_ratio_stats", "true"])
    GT.run_session(params, params["base_log_path"], backend=DenormEmu())
    names = [f for f in os.listdir(log_dir_of(params)) if f.endswith(".json") and f.startswith("band_ratio_")]
    assert sorted(names) == [f"band_ratio_shadowed_{s}.json" for s in (2, 4, 6)]


def test_a_device_resident_scene_is_sampled_where_it_is(tmp_path, monkeypatch):
    params = gan_params(tmp_path, "cycle_gan", ["--validate_while_training", "--pairing_method", "random"])
    params["path"] = GAN_SCENE + ":device=1"
    sets = []
    real = GT.read_hsi_data
    monkeypatch.setattr(GT, "read_hsi_data", lambda loader, data_set, *a, **k: (sets.append(data_set),
                                                                                real(loader, data_set, *a, **k))[1])
    host = gan_params(tmp_path / "host", "cycle_gan", ["--validate_while_training", "--pairing_method", "random"])
    # the same samples and pairs either way; the device prepares the scene in float32 launches of its own, an ulp
    # (6e-8) off the host's division here and there, and six training steps carry that along
    assert GT.run_session(params, params["base_log_path"], backend=DenormEmu()) == \
        pytest.approx(GT.run_session(host, host["base_log_path"], backend=DenormEmu()), rel=1e-5)
    assert sets[0].downloaded() == [] and type(sets[0]).__name__ == "DeviceBasicDataSet"


def test_only_the_chief_writes(tmp_path, monkeypatch):
    from hypelcnn_amd.classify import monitored_session_runner as M
    monkeypatch.setattr(M, "is_chief", lambda: False)
    params = gan_params(tmp_path, "cycle_gan", ["--validate_while_training"])
    result = GT.run_session(params, params["base_log_path"], backend=DenormEmu())
    assert len(result) == 2 and os.listdir(log_dir_of(params)) == []


# ----------------------------------------------------------------------------- 7. GAN study
def gan_study_argv(tmp_path, trials=2):
    overlay = tmp_path / "flags.json"
    overlay.write_text(json.dumps({"batch_size": 16, "validation_sample_count": 64}))
    return ["--loader_name", "SyntheticDataLoader", "--path", GAN_SCENE, "--step", "4", "--validation_steps", "2",
            "--base_log_path", str(tmp_path / "gan"), "--flag_config_file", str(overlay),
            "--flag_config_file_opt", os.path.join(OPT_DIR, "cycle_gan_flags_opt.json"),
            "--opt_trial_count", str(trials), "--opt_run_count", "1", "--opt_seed", "0",
            "--opt_storage", str(tmp_path / "study.db")]


def test_gan_study(tmp_path, capsys):
    study = GT.main(gan_study_argv(tmp_path), backend=DenormEmu())
    out = capsys.readouterr().out
    assert "Running on hyper parameter optimization mode" in out
    assert isinstance(study, H.Study) and study.study_name == "gan_shadow_opt"
    trials = study.trials
    assert [t.state for t in trials] == [H.COMPLETE] * 2 and all(math.isfinite(t.value) for t in trials)
    space = json.load(open(os.path.join(OPT_DIR, "cycle_gan_flags_opt.json")))
    for t in trials:
        assert t.params.keys() == {k for k, v in space.items() if isinstance(v, dict)}
        for key in ("generator_lr", "discriminator_lr"):
            assert space[key]["min"] <= t.params[key] <= space[key]["max"]
    dirs = [d for d in os.listdir(tmp_path) if d.startswith("gan_")]
    assert len(dirs) == 2
    for d in dirs:  # the study switches the hook on; the search space's constants win over the overlay, as in the reference
        assert "batch32" in d and {"best_ratio_shadowed.json", "best_ratio_deshadowed.json"} <= set(os.listdir(tmp_path / d))


def test_gan_study_is_refused_under_data_parallelism(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(GT, "run_session", lambda *a, **k: pytest.fail("a session ran"))
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        GT.main(gan_study_argv(tmp_path), backend=DenormEmu())
    assert not os.path.exists(tmp_path / "study.db")


# ----------------------------------------------------------------------------- episodes give back what they took
def test_an_episode_closes_its_session(tmp_path, monkeypatch):
    kept = {}
    real = GT._train_and_score

    def spy(*args):
        kept["ops"], kept["sess"] = args[-1], args[-1].ctx.session()
        out = real(*args)
        kept["towers"] = list(kept["sess"]._compiled.values())
        return out

    monkeypatch.setattr(GT, "_train_and_score", spy)
    params = gan_params(tmp_path, "cycle_gan", ["--validate_while_training"])
    GT.run_session(params, params["base_log_path"], backend=DenormEmu())
    ops, sess, towers = kept["ops"], kept["sess"], kept["towers"]
    assert ops.ctx._session is None and ops.pools == {} and ops.last_losses == {}
    assert sess._compiled == {} and sess.shared_inputs == {}
    assert all(getattr(sess, name) is None for name in ("params", "grads", "state", "slot_m", "slot_v"))
    assert len(towers) >= 4  # gen, dis, generate, validate_shadowed, validate_deshadowed
    for ct in towers:
        assert ct.plan is None and ct.fwd == () and ct.bwd == ()
        with pytest.raises(RuntimeError, match="closed"):
            ct.forward()
        with pytest.raises(RuntimeError, match="closed"):
            ct.forward_backward()
    sess.close()  # idempotent


def test_a_closed_tower_hands_its_graphs_back():
    from hypelcnn_amd.runtime import CompiledTower

    class Backend:
        destroyed = []

        def destroy_graph(self, replay):
            self.destroyed.append(replay.handle)
            replay.handle = None

    def graph(handle):
        def replay():
            pass
        replay.handle = handle
        return replay

    ct = CompiledTower.__new__(CompiledTower)
    ct.be, ct.plan, ct.fwd, ct.bwd = Backend(), object(), [1], [2]
    ct._captured = [graph(11), graph(12), graph(13)]
    ct._segments, ct._graph_fwd, ct._graph_all = [("run", ct._captured[0])], None, ct._captured[0]
    ct.close()
    assert Backend.destroyed == [11, 12, 13] and ct._captured == [] and ct._segments is None
    ct.close()
    assert Backend.destroyed == [11, 12, 13]
