"""Hyper-parameter search over whole training episodes: the reference's `objective()` rule (common/common_nn_ops.py:603-634)
and what it takes from optuna -- trials with suggest_float / suggest_int / suggest_categorical, a TPE sampler, a study
that minimises, resumable storage in one SQLite file.

optuna itself is not a dependency: the sampler is restated from its documented defaults and from Bergstra et al.,
"Algorithms for Hyper-Parameter Optimization" (NIPS 2011), and is not pinned against optuna's numbers; the storage
file has a schema of its own (DESIGN.md 3.14 lists the constants, the schema and the departures).  All of this is host
code: a trial costs a few hundred flops next to the training episode it schedules."""
import datetime
import json
import math
import os
import random
import sqlite3
import string
import zlib
from statistics import NormalDist

import numpy

RUNNING, COMPLETE, FAIL = "RUNNING", "COMPLETE", "FAIL"
SCHEMA_VERSION = 1
SCHEMA_TABLE = "hypel_opt_schema"

N_STARTUP_TRIALS = 10  # optuna's TPESampler defaults
N_EI_CANDIDATES = 24
GAMMA_SHARE, GAMMA_MAX = 0.1, 25
FLAT_WEIGHTS = 25
PRIOR_WEIGHT = 1.0
MAGIC_CLIP_KERNELS = 100
_NORMAL = NormalDist()
_EPS = 1e-12


# ----------------------------------------------------------------------------- distributions (plain dicts, JSON in the file)
def float_distribution(low, high, step=None, log=False):
    low, high = float(low), float(high)
    if step is not None and log:
        raise ValueError("suggest_float: `step` and `log` cannot be used together")
    if low > high:
        raise ValueError(f"suggest_float: low {low} is above high {high}")
    if log and low <= 0:
        raise ValueError(f"suggest_float: a log range needs low > 0, got {low}")
    if step is not None:
        step = float(step)
        if step <= 0:
            raise ValueError(f"suggest_float: step {step} is not positive")
        # the last grid point at or below `high` (a hair of slack for ranges such as 0.7 .. 2.7 by 0.1)
        high = low + math.floor((high - low) / step + 1e-9) * step
    return {"type": "float", "low": low, "high": high, "step": step, "log": bool(log)}


def int_distribution(low, high, step=1):
    low, high, step = int(low), int(high), int(step)
    if low > high:
        raise ValueError(f"suggest_int: low {low} is above high {high}")
    if step <= 0:
        raise ValueError(f"suggest_int: step {step} is not positive")
    return {"type": "int", "low": low, "high": low + (high - low) // step * step, "step": step}


def categorical_distribution(choices):
    choices = list(choices)
    if not choices:
        raise ValueError("suggest_categorical: no choices")
    return {"type": "categorical", "choices": choices}


def _model_range(dist):
    """(low, high) of the continuous axis a numeric parameter is modelled on: log space for `log`, widened by half a
    step for a grid."""
    low, high = float(dist["low"]), float(dist["high"])
    if dist.get("log"):
        return math.log(low), math.log(high)
    if dist.get("step"):
        return low - 0.5 * dist["step"], high + 0.5 * dist["step"]
    return low, high


def _to_model(dist, value):
    return math.log(value) if dist.get("log") else float(value)


def _from_model(dist, x):
    """Model axis -> a value of the distribution, never outside [low, high]."""
    low, high = dist["low"], dist["high"]
    if dist.get("log"):
        return min(max(math.exp(x), low), high)
    step = dist.get("step")
    if step:
        k = int(round((x - low) / step))
        k = min(max(k, 0), int(round((high - low) / step)))
        return low + k * step
    return min(max(x, low), high)


def _uniform_draw(dist, rng):
    if dist["type"] == "categorical":
        return dist["choices"][int(rng.integers(0, len(dist["choices"])))]
    lo, hi = _model_range(dist)
    return _from_model(dist, lo + (hi - lo) * float(rng.random()))


# ----------------------------------------------------------------------------- samplers
def _entropy_seed():
    return int.from_bytes(os.urandom(4), "little")


class RandomSampler:
    """Uniform over the space (log-uniform for `log` ranges, uniform over the grid points for grids).  Every draw has a
    generator of its own, keyed by (seed, trial number, parameter name): a resumed study goes on with new draws instead
    of repeating those of its first invocation, and two samplers with one seed agree trial by trial."""

    def __init__(self, seed=None):
        self.seed = _entropy_seed() if seed is None else int(seed)

    def rng_for(self, number, name, stream=0):
        return numpy.random.default_rng([self.seed, int(number), zlib.crc32(name.encode()), stream])

    def sample(self, trials, number, name, dist):
        return _uniform_draw(dist, self.rng_for(number, name))


def default_weights(n):
    """optuna's default_weights: equal up to 25 observations; beyond that the 25 newest keep 1 and the older ones ramp
    down linearly to 1 / n (oldest first)."""
    if n == 0:
        return numpy.zeros(0)
    if n < FLAT_WEIGHTS:
        return numpy.ones(n)
    return numpy.concatenate([numpy.linspace(1.0 / n, 1.0, n - FLAT_WEIGHTS), numpy.ones(FLAT_WEIGHTS)])


def _norm_cdf(z):
    return 0.5 * (1.0 + numpy.vectorize(math.erf, otypes=[float])(numpy.asarray(z, float) / math.sqrt(2.0)))


class _ParzenNumeric:
    """Mixture of one normal per observation, truncated to [low, high], plus the prior N((low + high) / 2, high - low)."""

    def __init__(self, obs, low, high):
        obs = numpy.asarray(obs, float)
        n = obs.size
        width = high - low
        mus = numpy.append(obs, 0.5 * (low + high))  # the prior is the last kernel
        if width <= 0:
            sigmas = numpy.ones(n + 1)
        else:
            order = numpy.argsort(mus, kind="stable")
            s = mus[order]
            sig_sorted = numpy.empty(n + 1)
            if n == 0:
                sig_sorted[:] = width
            else:  # neighbour distance: the farther of the two neighbours, the only neighbour at either end
                gaps = numpy.diff(s)
                sig_sorted[0], sig_sorted[-1] = gaps[0], gaps[-1]
                sig_sorted[1:-1] = numpy.maximum(gaps[:-1], gaps[1:])
            sigmas = numpy.empty(n + 1)
            sigmas[order] = sig_sorted
            sigmas[n] = width
            # "magic clip": no kernel narrower than the range over min(100, 1 + number of kernels)
            sigmas = numpy.clip(sigmas, width / min(MAGIC_CLIP_KERNELS, 1.0 + (n + 1)), width)
        w = numpy.append(default_weights(n), PRIOR_WEIGHT)
        self.low, self.high, self.mus, self.sigmas, self.weights = low, high, mus, sigmas, w / w.sum()
        self._cdf_lo = _norm_cdf((low - mus) / sigmas)
        self._mass = numpy.maximum(_norm_cdf((high - mus) / sigmas) - self._cdf_lo, _EPS)

    def sample(self, rng, count):
        which = rng.choice(self.mus.size, size=count, p=self.weights)
        u = rng.random(count)
        out = numpy.empty(count)
        for i, k in enumerate(which):
            p = min(max(self._cdf_lo[k] + u[i] * self._mass[k], _EPS), 1.0 - _EPS)
            out[i] = self.mus[k] + self.sigmas[k] * _NORMAL.inv_cdf(p)
        return numpy.clip(out, self.low, self.high)

    def log_pdf(self, xs):
        z = (numpy.asarray(xs, float)[:, None] - self.mus[None, :]) / self.sigmas[None, :]
        comp = numpy.log(self.weights)[None, :] - 0.5 * z * z - numpy.log(self.sigmas * math.sqrt(2.0 * math.pi))[None, :] \
            - numpy.log(self._mass)[None, :]
        top = comp.max(axis=1, keepdims=True)
        return (top + numpy.log(numpy.exp(comp - top).sum(axis=1, keepdims=True)))[:, 0]


class _ParzenCategorical:
    """Weighted counts of the observed choices plus the prior weight spread evenly."""

    def __init__(self, obs_index, n_choices):
        obs_index = numpy.asarray(obs_index, int)
        counts = numpy.full(n_choices, PRIOR_WEIGHT / n_choices)
        numpy.add.at(counts, obs_index, default_weights(obs_index.size))
        self.p = counts / counts.sum()

    def sample(self, rng, count):
        return rng.choice(self.p.size, size=count, p=self.p)

    def log_pdf(self, idx):
        return numpy.log(self.p[numpy.asarray(idx, int)])


class TPESampler(RandomSampler):
    """Tree-structured Parzen estimator, each parameter on its own (optuna's `multivariate=False`).  The first
    N_STARTUP_TRIALS completed trials are RandomSampler's draws for the same seed; afterwards the completed trials are
    split into the best gamma(n) = min(ceil(0.1 n), 25) and the rest, one Parzen estimator is fitted to each side, 24
    candidates are drawn from the better side's and the one with the largest log l(x) - log g(x) is suggested."""

    def sample(self, trials, number, name, dist):
        done = [t for t in trials if t.state == COMPLETE and t.value is not None]
        if len(done) < N_STARTUP_TRIALS:
            return super().sample(trials, number, name, dist)
        done.sort(key=lambda t: (t.value, t.number))
        n_below = min(int(math.ceil(GAMMA_SHARE * len(done))), GAMMA_MAX)
        # each side in trial order (the weights ramp over age); a trial that never drew this parameter, or drew it from
        # another distribution, tells nothing about it
        sides = []
        for side in (done[:n_below], done[n_below:]):
            side = sorted(side, key=lambda t: t.number)
            sides.append([t.params[name] for t in side if t.distributions.get(name) == dist])
        rng = self.rng_for(number, name, stream=1)
        if dist["type"] == "categorical":
            choices = dist["choices"]
            below, above = (_ParzenCategorical([choices.index(v) for v in obs], len(choices)) for obs in sides)
            cand = below.sample(rng, N_EI_CANDIDATES)
            return choices[int(cand[int(numpy.argmax(below.log_pdf(cand) - above.log_pdf(cand)))])]
        lo, hi = _model_range(dist)
        below, above = (_ParzenNumeric([_to_model(dist, v) for v in obs], lo, hi) for obs in sides)
        cand = below.sample(rng, N_EI_CANDIDATES)
        best = float(cand[int(numpy.argmax(below.log_pdf(cand) - above.log_pdf(cand)))])
        value = _from_model(dist, best)
        return int(round(value)) if dist["type"] == "int" else value


def get_sampler(name, seed=None):
    samplers = {"tpe": TPESampler, "random": RandomSampler}
    if name not in samplers:
        raise ValueError(f"unknown sampler {name!r}: one of {sorted(samplers)}")
    return samplers[name](seed)


# ----------------------------------------------------------------------------- trials
class FrozenTrial:
    """A stored trial: number, state, value, params (name -> value) and distributions (name -> dict)."""

    def __init__(self, number, state, value, params, distributions):
        self.number, self.state, self.value = number, state, value
        self.params, self.distributions = params, distributions

    def __repr__(self):
        return f"FrozenTrial(number={self.number}, state={self.state}, value={self.value}, params={self.params})"


class Trial:
    """What the objective gets: the suggest_* calls of optuna's Trial.  A name suggested twice gives the same value."""

    def __init__(self, study, trial_id, number):
        self.study, self._trial_id, self.number = study, trial_id, number
        self.params, self.distributions = {}, {}
        self._history = None

    def _suggest(self, name, dist):
        if name in self.params:
            if self.distributions[name] != dist:
                raise ValueError(f"parameter {name!r} was already suggested from {self.distributions[name]}")
            return self.params[name]
        if self._history is None:  # read once per trial: nothing completes while it runs (one worker per file)
            self._history = self.study.completed_trials()
        value = self.study.sampler.sample(self._history, self.number, name, dist)
        if dist["type"] == "int":
            value = int(round(value))
        elif dist["type"] == "float":
            value = float(value)
        self.params[name], self.distributions[name] = value, dist  # (written with the trial's verdict: Study.tell)
        return value

    def suggest_float(self, name, low, high, step=None, log=False):
        return self._suggest(name, float_distribution(low, high, step, log))

    def suggest_int(self, name, low, high, step=1):
        return self._suggest(name, int_distribution(low, high, step))

    def suggest_categorical(self, name, choices):
        return self._suggest(name, categorical_distribution(choices))

    def random(self, tag):
        """A `random.Random` of this trial, from the study's seed: the same study seed, trial number and tag give the
        same stream; Python's global generator is not touched."""
        return random.Random(f"{self.study.sampler.seed}:{self.number}:{tag}")


# ----------------------------------------------------------------------------- storage + study
_DDL = (
    f"CREATE TABLE {SCHEMA_TABLE} (version INTEGER NOT NULL)",
    "CREATE TABLE studies (study_id INTEGER PRIMARY KEY, study_name TEXT NOT NULL UNIQUE, direction TEXT NOT NULL)",
    "CREATE TABLE trials (trial_id INTEGER PRIMARY KEY, study_id INTEGER NOT NULL REFERENCES studies(study_id), "
    "number INTEGER NOT NULL, state TEXT NOT NULL, value REAL, datetime_start TEXT, datetime_complete TEXT, "
    "UNIQUE (study_id, number))",
    "CREATE TABLE trial_params (trial_id INTEGER NOT NULL REFERENCES trials(trial_id), param_name TEXT NOT NULL, "
    "param_value TEXT NOT NULL, distribution_json TEXT NOT NULL, PRIMARY KEY (trial_id, param_name))",
)


def _check_file(path):
    """Refuse a file that is not ours BEFORE anything is written: opened read-only, its table list must be empty (a new
    file) or hold our schema table.  -> whether the schema has to be created."""
    if not os.path.exists(path) or os.path.getsize(path) == 0:
        return True
    try:
        con = sqlite3.connect(f"file:{os.path.abspath(path)}?mode=ro", uri=True)
        try:
            tables = [r[0] for r in con.execute("SELECT name FROM sqlite_master WHERE type = 'table'")]
            version = con.execute(f"SELECT version FROM {SCHEMA_TABLE}").fetchone() if SCHEMA_TABLE in tables else None
        finally:
            con.close()
    except sqlite3.DatabaseError as e:
        raise ValueError(f"{path} is not a study file of this package ({e}); it is left as it is") from e
    if SCHEMA_TABLE not in tables:
        if not tables:
            return True
        raise ValueError(f"{path} is an SQLite file without this package's study schema (tables: {sorted(tables)}) -- "
                         f"an optuna database, for one, is not read; it is left as it is. Pass another --opt_storage")
    if version is None or version[0] != SCHEMA_VERSION:
        raise ValueError(f"{path} holds study schema version {version and version[0]}, this package reads {SCHEMA_VERSION}")
    return False


def _now():
    return datetime.datetime.now().isoformat(timespec="seconds")


class Study:
    """direction: minimize (the only one the reference uses)."""

    def __init__(self, study_name, storage_path, sampler, con, study_id):
        self.study_name, self.storage_path, self.sampler = study_name, storage_path, sampler
        self._con, self._study_id = con, study_id
        self._completed = None  # read from the file once, then kept up to date by tell(): one worker per file

    # ---- storage ----
    def _load(self, where="", args=()):
        rows = self._con.execute(f"SELECT trial_id, number, state, value FROM trials WHERE study_id = ? {where} "
                                 f"ORDER BY number", (self._study_id,) + tuple(args)).fetchall()
        out = [(trial_id, FrozenTrial(number, state, value, {}, {})) for trial_id, number, state, value in rows]
        by_id = dict(out)
        for trial_id, name, v, d in self._con.execute(
                "SELECT p.trial_id, p.param_name, p.param_value, p.distribution_json FROM trial_params p JOIN trials t "
                "ON t.trial_id = p.trial_id WHERE t.study_id = ?", (self._study_id,)):
            if trial_id in by_id:
                by_id[trial_id].params[name], by_id[trial_id].distributions[name] = json.loads(v), json.loads(d)
        return [t for _, t in out]

    @property
    def trials(self):
        return self._load()

    def completed_trials(self):
        """What the sampler learns from: COMPLETE trials only (a RUNNING row left by a killed process and FAIL trials
        are ignored)."""
        if self._completed is None:
            self._completed = self._load("AND state = ?", (COMPLETE,))
        return list(self._completed)

    @property
    def best_trial(self):
        done = self.completed_trials()
        if not done:
            raise ValueError(f"study {self.study_name!r} has no completed trial")
        return min(done, key=lambda t: (t.value, t.number))

    @property
    def best_value(self):
        return self.best_trial.value

    @property
    def best_params(self):
        return self.best_trial.params

    # ---- trials ----
    def ask(self):
        """A new RUNNING trial with the next number."""
        with self._con:
            number = self._con.execute("SELECT COALESCE(MAX(number), -1) + 1 FROM trials WHERE study_id = ?",
                                       (self._study_id,)).fetchone()[0]
            cur = self._con.execute("INSERT INTO trials (study_id, number, state, datetime_start) VALUES (?, ?, ?, ?)",
                                    (self._study_id, number, RUNNING, _now()))
        return Trial(self, cur.lastrowid, number)

    def tell(self, trial, value=None, state=None):
        """Close a trial.  A value that is None or NaN makes it FAIL."""
        value = None if value is None else float(value)
        if state is None:
            state = FAIL if value is None or math.isnan(value) else COMPLETE
        if state != COMPLETE:
            value = None
        with self._con:  # one transaction: the parameters and the verdict
            self._con.executemany("INSERT INTO trial_params VALUES (?, ?, ?, ?)",
                                  [(trial._trial_id, name, json.dumps(v), json.dumps(trial.distributions[name]))
                                   for name, v in trial.params.items()])
            self._con.execute("UPDATE trials SET state = ?, value = ?, datetime_complete = ? WHERE trial_id = ?",
                              (state, value, _now(), trial._trial_id))
        if state == COMPLETE and self._completed is not None:
            self._completed.append(FrozenTrial(trial.number, state, value, dict(trial.params), dict(trial.distributions)))
        return state

    def add_trial(self, params, distributions, value):
        """Record a finished trial that ran elsewhere (optuna's add_trial)."""
        trial = self.ask()
        trial.params, trial.distributions = dict(params), {name: distributions[name] for name in params}
        self.tell(trial, value)
        return trial.number

    def optimize(self, func, n_trials, callbacks=()):
        """Run `n_trials` more trials of func(trial) -> value.  A trial whose function raises is marked FAIL and the
        exception propagates (optuna's catch=()); a NaN value marks it FAIL and the study goes on.
        callbacks: called as callback(study, frozen_trial) after each trial."""
        for _ in range(int(n_trials)):
            trial = self.ask()
            try:
                value = func(trial)
            except BaseException:
                self.tell(trial, state=FAIL)
                raise
            state = self.tell(trial, value)
            if state == COMPLETE:
                best = self.best_trial
                print(f"Trial {trial.number} finished with value: {float(value)} and parameters: {trial.params}. "
                      f"Best is trial {best.number} with value: {best.value}.")
            else:
                print(f"Trial {trial.number} failed with parameters: {trial.params} because of the following error: "
                      f"The value {value} is not acceptable.")
            for cb in callbacks:
                cb(self, FrozenTrial(trial.number, state, value if state == COMPLETE else None, dict(trial.params),
                                     dict(trial.distributions)))
        return self

    def close(self):
        self._con.close()


def default_storage_path(study_name):
    """<study_name>.db in the working directory: where the reference's `sqlite:///<study_name>.db` lands."""
    return os.path.join(os.getcwd(), f"{study_name}.db")


def create_study(study_name, storage_path=None, sampler=None, load_if_exists=True):
    storage_path = default_storage_path(study_name) if storage_path is None else os.fspath(storage_path)
    fresh = _check_file(storage_path)
    con = sqlite3.connect(storage_path)
    with con:
        if fresh:
            for ddl in _DDL:
                con.execute(ddl)
            con.execute(f"INSERT INTO {SCHEMA_TABLE} VALUES (?)", (SCHEMA_VERSION,))
        row = con.execute("SELECT study_id FROM studies WHERE study_name = ?", (study_name,)).fetchone()
        if row is None:
            study_id = con.execute("INSERT INTO studies (study_name, direction) VALUES (?, 'minimize')",
                                   (study_name,)).lastrowid
        elif load_if_exists:
            study_id = row[0]
    if row is not None and not load_if_exists:
        con.close()
        raise ValueError(f"study {study_name!r} already exists in {storage_path}")
    return Study(study_name, storage_path, sampler if sampler is not None else TPESampler(), con, study_id)


# ----------------------------------------------------------------------------- the reference's objective
def apply_search_space(trial, params, params_from_json_opt):
    """The reference's rule, entry by entry: {min, max} of floats -> suggest_float (step / log from the entry), of ints
    -> suggest_int; mixed types keep the default; a list -> categorical; anything else overrides the parameter."""
    for key, value in params_from_json_opt.items():
        if type(value) is dict:
            if "min" in value and "max" in value:
                min_range_val, max_range_val = value["min"], value["max"]
                if type(min_range_val) is float and type(max_range_val) is float:
                    params[key] = trial.suggest_float(key, min_range_val, max_range_val, step=value.get("step"),
                                                      log=value.get("log", False))
                elif type(min_range_val) is int and type(max_range_val) is int:
                    params[key] = trial.suggest_int(key, min_range_val, max_range_val, step=value.get("step", 1))
                else:
                    print(f"Parameter value is put in hyper optimization "
                          f"config but its min max type is inconsistent: {key}. "
                          f"Using the default value")
        elif type(value) is list:
            params[key] = trial.suggest_categorical(key, value)
        else:
            params[key] = value
    return params


def objective(trial, params, params_from_json_opt, func_to_run, opt_run_count, base_log_path):
    """One trial = `opt_run_count` whole episodes with the suggested parameters, each in a log directory of its own; the
    trial's value is the WORST (largest) of the runs' mean results."""
    apply_search_space(trial, params, params_from_json_opt)
    rng = trial.random("log_path")
    losses = []
    for run_idx in range(0, opt_run_count):
        trial_postfix = "_" + "".join(rng.choices(string.ascii_lowercase + string.digits, k=5))
        print(f"Starting run#{run_idx}")
        losses.append(numpy.mean(func_to_run(params=params, base_log_path=base_log_path + trial_postfix)))
    print("Trial runs are completed. Losses:")
    print(*losses, sep=",")
    return max(losses)


def refuse_data_parallel(what):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError(f"{what}: a hyper-parameter study under WORLD_SIZE > 1 is not provided -- every rank "
                                  f"would have to draw the same trial, and that rendezvous is not built. Run the study on "
                                  f"one device")
