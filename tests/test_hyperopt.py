"""CPU: the hyper-parameter search of common/hyperopt.py -- the reference's space rule on its three search spaces and
ours, `objective`, the two samplers (TPE against the random baseline, never against a stored number) and the SQLite
storage with resume."""
import json
import math
import os
import re
import sqlite3

import numpy as np
import pytest

from hypelcnn_amd.common import hyperopt as H

OPT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "opt")
SPACES = ["cycle_gan_flags_opt.json", "dcl_gan_flags_opt.json", "dcl_cycle_gan_flags_opt.json",
          "classification_opt_small.json"]
MIXED_MESSAGE = "Parameter value is put in hyper optimization config but its min max type is inconsistent: {}. " \
                "Using the default value"


def _study(tmp_path, sampler, name="s", file="study.db"):
    return H.create_study(name, str(tmp_path / file), sampler)


def _float_dist(low, high, **kw):
    return H.float_distribution(low, high, **kw)


# ----------------------------------------------------------------------------- 1. the space rule
@pytest.fixture(scope="module")
def drawn(tmp_path_factory):
    """200 seeded trials of every space with either sampler, run once: {(space, sampler): [params of each trial]}.
    The value steers TPE somewhere, so that its model-based draws are exercised as well."""
    out = {}
    for space_name in SPACES:
        space = json.load(open(os.path.join(OPT_DIR, space_name)))
        ranged = sorted(k for k, v in space.items() if isinstance(v, dict) and type(v["min"]) is float)
        for sampler in (H.RandomSampler(7), H.TPESampler(7)):
            study = H.create_study("space", str(tmp_path_factory.mktemp("space") / "s.db"), sampler)
            seen = []

            def func(trial):
                params = H.apply_search_space(trial, {"batch_size": -1, "untouched": "kept"}, space)
                seen.append(params)
                return sum(params[k] for k in ranged)

            study.optimize(func, 200)
            out[space_name, type(sampler).__name__] = seen
    return out


@pytest.mark.parametrize("sampler", ["RandomSampler", "TPESampler"])
@pytest.mark.parametrize("space_name", SPACES)
def test_every_draw_obeys_the_space(drawn, space_name, sampler):
    space = json.load(open(os.path.join(OPT_DIR, space_name)))
    trials = drawn[space_name, sampler]
    assert len(trials) == 200
    for params in trials:
        assert params["untouched"] == "kept"
        for key, entry in space.items():
            v = params[key]
            if isinstance(entry, dict):
                lo, hi = entry["min"], entry["max"]
                assert lo <= v <= hi, (key, v)
                if type(lo) is int:
                    assert type(v) is int, (key, v)
                else:
                    assert type(v) is float, (key, v)
                if "step" in entry:
                    k = round((v - lo) / entry["step"])
                    assert v == pytest.approx(lo + k * entry["step"], rel=1e-9, abs=0), (key, v)
            elif isinstance(entry, list):
                assert v in entry
            else:
                assert v == entry and type(v) is type(entry), key  # a constant overrides the parameter
    if space_name != "classification_opt_small.json":
        assert {p["gan_type"] for p in trials} == {space["gan_type"]}
        assert {p["batch_size"] for p in trials} == {32} and {p["validation_sample_count"] for p in trials} == {600}
    if space_name.startswith("dcl"):
        assert {p["embedded_feat_size"] for p in trials} <= {1, 2, 3, 4} and {p["patches"] for p in trials} <= {4, 5, 6, 7, 8}
        if sampler == "RandomSampler":  # both ends are reachable
            assert {p["embedded_feat_size"] for p in trials} == {1, 2, 3, 4}
            assert {p["patches"] for p in trials} == {4, 5, 6, 7, 8}
    # identity_loss_weight 0.5 .. 2.0 by 0.2: `high` is lowered to the last grid point, 1.9
    if "identity_loss_weight" in space:
        assert max(p["identity_loss_weight"] for p in trials) <= 1.9 + 1e-9


@pytest.mark.parametrize("space_name", SPACES)
def test_log_parameters_are_uniform_in_the_logarithm(drawn, space_name):
    space = json.load(open(os.path.join(OPT_DIR, space_name)))
    logs = [k for k, v in space.items() if isinstance(v, dict) and v.get("log")]
    assert logs
    for key in logs:
        mid = math.sqrt(space[key]["min"] * space[key]["max"])
        share = np.mean([p[key] < mid for p in drawn[space_name, "RandomSampler"]])
        assert 0.36 <= share <= 0.64, (key, share)  # 0.5 +- 4 standard deviations of a 200-draw binomial


def test_mixed_types_keep_the_default_and_say_so(tmp_path, capsys):
    trial = _study(tmp_path, H.RandomSampler(0)).ask()
    params = H.apply_search_space(trial, {"a": "default", "b": "default", "c": 5},
                                  {"a": {"min": 1, "max": 2.0}, "b": {"max": 3.0}, "c": {"min": 1, "max": 9, "step": 4}})
    assert params["a"] == "default"
    assert MIXED_MESSAGE.format("a") in capsys.readouterr().out
    assert params["b"] == "default"  # a dict without `min` changes nothing
    assert params["c"] in (1, 5, 9) and "a" not in trial.params and "b" not in trial.params


def test_step_with_log_raises_and_ranges_are_checked(tmp_path):
    trial = _study(tmp_path, H.RandomSampler(0)).ask()
    with pytest.raises(ValueError, match="step.*log"):
        trial.suggest_float("x", 0.1, 1.0, step=0.1, log=True)
    with pytest.raises(ValueError, match="step.*log"):
        H.apply_search_space(trial, {}, {"x": {"min": 0.1, "max": 1.0, "step": 0.1, "log": True}})
    with pytest.raises(ValueError, match="low > 0"):
        trial.suggest_float("y", 0.0, 1.0, log=True)
    assert trial.suggest_int("i", 3, 3) == 3
    assert trial.suggest_float("z", 0.5, 2.0, step=0.2) <= 1.9 + 1e-9
    assert trial.suggest_float("z", 0.5, 2.0, step=0.2) == trial.params["z"]  # asked twice: the same value


# ----------------------------------------------------------------------------- 2. objective
def test_objective_runs_the_episodes_and_returns_the_worst_mean(tmp_path, capsys):
    def run(seed, sub):
        calls = []
        results = iter([[0.1, 0.3], 0.5, [0.4, 0.2]])

        def func_to_run(params, base_log_path):
            calls.append((dict(params), base_log_path))
            return next(results)

        trial = _study(tmp_path, H.RandomSampler(seed), file=sub).ask()
        value = H.objective(trial, {"lr": 1.0, "k": 0}, {"lr": {"min": 0.1, "max": 0.2}, "k": 3}, func_to_run, 3, "/logs/base")
        return value, calls

    value, calls = run(5, "a.db")
    out = capsys.readouterr().out
    assert value == pytest.approx(0.5)  # means 0.2, 0.5, 0.3: the maximum
    assert len(calls) == 3
    paths = [p for _, p in calls]
    assert len(set(paths)) == 3 and all(re.fullmatch(r"/logs/base_[a-z0-9]{5}", p) for p in paths), paths
    assert all(0.1 <= params["lr"] <= 0.2 and params["k"] == 3 for params, _ in calls)
    assert "Starting run#0" in out and "Starting run#2" in out and "Trial runs are completed. Losses:" in out
    assert [p for _, p in run(5, "b.db")[1]] == paths  # the same seed: the same paths
    assert [p for _, p in run(6, "c.db")[1]] != paths


def test_objective_leaves_pythons_global_generator_alone(tmp_path):
    import random
    random.seed(11)
    want = random.random()
    random.seed(11)
    H.objective(_study(tmp_path, H.RandomSampler(0)).ask(), {}, {}, lambda params, base_log_path: 0.0, 2, "x")
    assert random.random() == want


# ----------------------------------------------------------------------------- 3. samplers
def _two_param(trial):
    return (trial.suggest_float("x", 0.0, 1.0) - 0.3) ** 2 + \
        (math.log10(trial.suggest_float("y", 1e-5, 1e-1, log=True)) + 2) ** 2


def test_startup_trials_are_the_random_samplers_draws(tmp_path):
    tpe, rnd = _study(tmp_path, H.TPESampler(3), file="t.db"), _study(tmp_path, H.RandomSampler(3), file="r.db")
    tpe.optimize(_two_param, 14)
    rnd.optimize(_two_param, 14)
    a, b = [t.params for t in tpe.trials], [t.params for t in rnd.trials]
    assert a[:10] == b[:10]
    assert all(a[i] != b[i] for i in range(10, 14))


def test_known_answer_tpe_suggests_near_the_minimum(tmp_path):
    dist = _float_dist(0.0, 1.0)
    study = _study(tmp_path, H.RandomSampler(0))
    for x in np.random.default_rng(0).random(30):
        study.add_trial({"x": float(x)}, {"x": dist}, (float(x) - 0.2) ** 2)
    history = study.completed_trials()
    assert len(history) == 30
    tpe = [H.TPESampler(seed).sample(history, 30, "x", dist) for seed in range(50)]
    rnd = [H.RandomSampler(seed).sample(history, 30, "x", dist) for seed in range(50)]
    assert all(0.0 <= v <= 1.0 for v in tpe)
    assert abs(np.median(tpe) - 0.2) < abs(np.median(rnd) - 0.2), (np.median(tpe), np.median(rnd))
    assert len(study.completed_trials()) == 30  # the suggestions were not added


def test_tpe_beats_the_random_baseline(tmp_path):
    best = {"TPESampler": [], "RandomSampler": []}
    for seed in range(10):
        for sampler in (H.TPESampler(seed), H.RandomSampler(seed)):
            study = _study(tmp_path, sampler, file=f"{type(sampler).__name__}{seed}.db")
            study.optimize(_two_param, 60)
            best[type(sampler).__name__].append(study.best_value)
    tpe, rnd = np.median(best["TPESampler"]), np.median(best["RandomSampler"])
    print(f"median best of 60 trials, seeds 0..9: TPE {tpe:.6g}, random {rnd:.6g}")
    assert tpe < rnd, (tpe, rnd)


def test_tpe_prefers_the_good_category(tmp_path):
    choices = ["a", "b", "c", "d"]
    dist = H.categorical_distribution(choices)
    study = _study(tmp_path, H.RandomSampler(0))
    for i in range(30):
        c = choices[i % 4]
        study.add_trial({"c": c}, {"c": dist}, 0.0 if c == "c" else 1.0 + 0.01 * i)
    picks = [H.TPESampler(seed).sample(study.completed_trials(), 30, "c", dist) for seed in range(50)]
    assert picks.count("c") / 50 > 1 / len(choices), picks


def test_weights_ramp_down_for_old_observations():
    assert (H.default_weights(24) == 1).all() and H.default_weights(0).size == 0
    w = H.default_weights(40)
    assert w.size == 40 and (w[-25:] == 1).all() and w[0] == pytest.approx(1 / 40) and (np.diff(w[:15]) > 0).all()


# ----------------------------------------------------------------------------- 4. storage
class CountingSampler(H.RandomSampler):
    def __init__(self, seed):
        super().__init__(seed)
        self.saw = {}

    def sample(self, trials, number, name, dist):
        self.saw[number] = [t.number for t in trials]
        return super().sample(trials, number, name, dist)


def _one_param(trial):
    return (trial.suggest_float("x", -1.0, 1.0) - 0.25) ** 2


def test_a_second_invocation_continues_the_study(tmp_path, capsys):
    first = _study(tmp_path, H.RandomSampler(1))
    first.optimize(_one_param, 10)
    assert re.search(r"Trial 9 finished with value: \S+ and parameters: \{'x': \S+\}\. Best is trial \d with value: \S+\.",
                     capsys.readouterr().out)
    first.close()
    con = sqlite3.connect(str(tmp_path / "study.db"))
    with con:  # what a killed process leaves behind
        con.execute("INSERT INTO trials (study_id, number, state, value) VALUES (1, 10, 'RUNNING', NULL)")
    con.close()
    sampler = CountingSampler(1)
    second = _study(tmp_path, sampler)
    second.optimize(_one_param, 10)
    trials = second.trials
    assert [t.number for t in trials] == list(range(21))
    assert [t.state for t in trials] == [H.COMPLETE] * 10 + [H.RUNNING] + [H.COMPLETE] * 10
    assert sampler.saw[11] == list(range(10))  # the first new trial saw the ten completed ones, not the RUNNING row
    assert sampler.saw[20] == list(range(10)) + list(range(11, 20))
    done = [t for t in trials if t.state == H.COMPLETE]
    assert second.best_value == min(t.value for t in done)
    assert second.best_trial.number == min(done, key=lambda t: t.value).number
    assert second.best_params == second.best_trial.params
    # a resumed study draws anew: the second ten are not the first ten again
    assert {t.params["x"] for t in done[:10]}.isdisjoint(t.params["x"] for t in done[10:])


def test_numbers_run_on_without_a_gap_when_nothing_was_left_running(tmp_path):
    _study(tmp_path, H.RandomSampler(1)).optimize(_one_param, 10)
    sampler = CountingSampler(1)
    study = _study(tmp_path, sampler)
    study.optimize(_one_param, 10)
    assert [t.number for t in study.trials] == list(range(20))
    assert sampler.saw[10] == list(range(10))
    assert study.best_value == min(t.value for t in study.trials)


def test_a_raising_trial_fails_and_propagates_a_nan_trial_fails_and_goes_on(tmp_path, capsys):
    study = _study(tmp_path, H.RandomSampler(2))

    def func(trial):
        x = trial.suggest_float("x", 0.0, 1.0)
        if trial.number == 1:
            return float("nan")
        if trial.number == 3:
            raise RuntimeError("episode broke")
        return x

    with pytest.raises(RuntimeError, match="episode broke"):
        study.optimize(func, 6)
    assert [t.state for t in study.trials] == [H.COMPLETE, H.FAIL, H.COMPLETE, H.FAIL]
    assert "Trial 1 failed" in capsys.readouterr().out
    assert [t.number for t in study.completed_trials()] == [0, 2]
    assert study.trials[3].params.keys() == {"x"} and study.trials[1].value is None
    with pytest.raises(ValueError, match="no completed trial"):
        _study(tmp_path, H.RandomSampler(0), name="empty").best_trial


def test_a_foreign_sqlite_file_is_refused_and_left_alone(tmp_path):
    path = tmp_path / "gan_shadow_opt.db"
    con = sqlite3.connect(str(path))
    with con:  # the tables an optuna database starts with
        con.execute("CREATE TABLE studies (study_id INTEGER PRIMARY KEY, study_name VARCHAR(512))")
        con.execute("CREATE TABLE alembic_version (version_num VARCHAR(32))")
    con.close()
    before = path.read_bytes()
    with pytest.raises(ValueError, match=re.escape(str(path))):
        H.create_study("gan_shadow_opt", str(path), H.RandomSampler(0))
    assert path.read_bytes() == before and sorted(os.listdir(tmp_path)) == ["gan_shadow_opt.db"]
    text = tmp_path / "notes.db"
    text.write_text("not a database at all, but long enough to be read as a header " * 4)
    with pytest.raises(ValueError, match=re.escape(str(text))):
        H.create_study("s", str(text), H.RandomSampler(0))
    assert text.read_text().startswith("not a database")


def test_the_default_file_is_the_study_name_in_the_working_directory(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    study = H.create_study("classification_opt", sampler=H.RandomSampler(0))
    study.optimize(_one_param, 1)
    assert os.listdir(tmp_path) == ["classification_opt.db"]
    assert study.storage_path == str(tmp_path / "classification_opt.db")
    with pytest.raises(ValueError, match="already exists"):
        H.create_study("classification_opt", sampler=H.RandomSampler(0), load_if_exists=False)


def test_two_studies_share_a_file(tmp_path):
    a, b = _study(tmp_path, H.RandomSampler(0), name="a"), _study(tmp_path, H.RandomSampler(0), name="b")
    a.optimize(_one_param, 3)
    b.optimize(_one_param, 2)
    assert [t.number for t in a.trials] == [0, 1, 2] and [t.number for t in b.trials] == [0, 1]


def test_the_flags(tmp_path):
    from hypelcnn_amd.classify import train_for_classification as T
    from hypelcnn_amd.gan import gan_train_for_shadow as GT
    for parser in (T.build_parser(), GT.build_parser()):
        flags, _ = parser.parse_known_args([])
        assert (flags.flag_config_file_opt, flags.opt_trial_count, flags.opt_run_count) == (None, 10, 3)
        assert (flags.opt_seed, flags.opt_sampler, flags.opt_storage) == (None, "tpe", None)
        flags, _ = parser.parse_known_args(["--opt_seed", "4", "--opt_sampler", "random", "--opt_storage", "x.db"])
        assert (flags.opt_seed, flags.opt_sampler, flags.opt_storage) == (4, "random", "x.db")
    assert GT.build_parser().parse_known_args([])[0].validate_while_training is False
    assert isinstance(H.get_sampler("tpe", 1), H.TPESampler) and type(H.get_sampler("random", 1)) is H.RandomSampler
    with pytest.raises(ValueError, match="unknown sampler"):
        H.get_sampler("grid")
