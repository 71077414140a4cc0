#!/usr/bin/env python3
"""Pin utilities/stat_extractor.py by executing the reference's own functions (build container only; needs
/root/reference).

`utilities/stat_extractor.py` runs UNCHANGED: calc_kappa, extract_accuracy_metrics, extract_statistics_info and
calculate_mean_std_metrics on three small confusion matrices, one of them with an empty class row (a NaN class
accuracy, stored as null).  Written to tests/golden/reference_stat_extractor.json; only data is written."""
import importlib
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

MATRICES = [
    [[50, 2, 1], [3, 40, 7], [0, 5, 30]],
    [[12, 0, 3, 1], [0, 0, 0, 0], [2, 1, 20, 0], [4, 0, 0, 9]],  # class 1 has no samples
    [[7, 1, 0], [2, 9, 3], [1, 0, 11]],
]


def _plain(v):
    a = np.asarray(v, dtype=float)
    return np.where(np.isnan(a), None, a.astype(object)).tolist()


def main():
    if not os.path.isdir(REF):
        raise RuntimeError("the reference is only present in the build container")
    np.int = int
    sys.path.insert(0, os.path.join(REF, "utilities"))
    ref = importlib.import_module("stat_extractor")
    assert os.path.abspath(ref.__file__).startswith(REF)
    mats = [np.asarray(m, dtype=int) for m in MATRICES]
    out = {"matrices": MATRICES, "per_matrix": []}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for m in mats:
            oa, aa, kappa, samples = ref.extract_accuracy_metrics(m)
            out["per_matrix"].append({"kappa": float(ref.calc_kappa(m)), "overall_accuracy": float(oa),
                                      "class_accuracy": _plain(aa), "metrics_kappa": float(kappa),
                                      "class_based_samples": [int(s) for s in samples]})
        same_shape = [mats[0], mats[2]]
        holder = ref.extract_statistics_info(same_shape)
        out["statistics"] = {"inputs": [0, 2], "oa_array": _plain(holder.oa_array), "aa_array": _plain(holder.aa_array),
                             "kappa_array": _plain(holder.kappa_array),
                             "sample_count": [int(s) for s in holder.sample_count],
                             "mean_std": _plain(ref.calculate_mean_std_metrics(holder.oa_array, holder.aa_array,
                                                                               holder.kappa_array))}
        single = ref.extract_statistics_info([mats[1]])
        out["statistics_empty_row"] = {"inputs": [1], "oa_array": _plain(single.oa_array),
                                       "aa_array": _plain(single.aa_array), "kappa_array": _plain(single.kappa_array),
                                       "sample_count": [int(s) for s in single.sample_count]}
    with open(os.path.join(HERE, "reference_stat_extractor.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
