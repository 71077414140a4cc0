"""CPU: utilities/stat_extractor.py against the recorded results of the reference's own functions
(tests/golden/reference_stat_extractor.json, written by tests/golden/make_reference_stat_extractor.py), and calc_kappa
against the vectorised kappa of classify/classic_ml_trainer.scores."""
import json
import os

import numpy as np
import pytest

from hypelcnn_amd.utilities import stat_extractor as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_stat_extractor.json")
TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return json.load(open(GOLDEN))


def close(got, want):
    got = np.asarray(got, dtype=float)
    want = np.asarray([[np.nan if x is None else x for x in row] if isinstance(row, list) else
                       (np.nan if row is None else row) for row in want] if isinstance(want, list) else want,
                      dtype=float)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and \
        bool((np.abs(got - want)[~np.isnan(want)] <= TOL).all())


def test_per_matrix_metrics_match_the_reference(gold):
    assert any(0 in np.asarray(m).sum(axis=1) for m in gold["matrices"])  # the empty class row is among them
    for m, want in zip(gold["matrices"], gold["per_matrix"]):
        m = np.asarray(m, dtype=int)
        assert abs(S.calc_kappa(m) - want["kappa"]) <= TOL
        oa, aa, kappa, samples = S.extract_accuracy_metrics(m)
        assert abs(oa - want["overall_accuracy"]) <= TOL and abs(kappa - want["metrics_kappa"]) <= TOL
        assert close(aa, want["class_accuracy"])
        assert samples.tolist() == want["class_based_samples"]
        assert S.histogram(m, 0).tolist() == m.sum(axis=1).tolist() and S.histogram(m, 1).tolist() == m.sum(axis=0).tolist()


def test_statistics_match_the_reference(gold):
    for key in ("statistics", "statistics_empty_row"):
        want = gold[key]
        holder = S.extract_statistics_info([np.asarray(gold["matrices"][i], dtype=int) for i in want["inputs"]])
        assert close(holder.oa_array, want["oa_array"]) and close(holder.aa_array, want["aa_array"])
        assert close(holder.kappa_array, want["kappa_array"])
        assert holder.sample_count.tolist() == want["sample_count"]
        if "mean_std" in want:
            assert close(S.calculate_mean_std_metrics(holder.oa_array, holder.aa_array, holder.kappa_array),
                         want["mean_std"])


def test_first_run_lands_in_the_last_slot():
    a, b, c = (np.asarray(m) for m in ([[9, 1], [1, 9]], [[5, 5], [5, 5]], [[10, 0], [0, 10]]))
    holder = S.extract_statistics_info([a, b, c])
    assert holder.oa_array.tolist() == [0.5, 1.0, 0.9]  # index - 1: run 0 at [-1]
    assert holder.sample_count.tolist() == [10, 10]


def test_calc_kappa_equals_the_trainer_scores(gold):
    from hypelcnn_amd.classify.classic_ml_trainer import scores
    rng = np.random.default_rng(0)
    mats = [np.asarray(m) for m in gold["matrices"]] + [rng.integers(0, 50, (7, 7))]
    for m in mats:
        assert abs(S.calc_kappa(m) - scores(m)[2]) <= TOL


def test_csv_directory_round_trip(tmp_path, capsys):
    for i, m in enumerate(([[9, 1], [1, 9]], [[5, 5], [5, 5]])):
        np.savetxt(tmp_path / f"m{i}.csv", np.asarray(m), fmt="%d", delimiter=",")
    S.main([str(tmp_path)])
    out = capsys.readouterr().out
    assert "OA: 0.9000" in out and "OA: 0.5000" in out and "#Class based accuracy" in out
