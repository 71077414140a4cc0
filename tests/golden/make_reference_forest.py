"""Writes tests/golden/reference_forest.json / .npz with scikit-learn (run from the repository root:
`python -m tests.golden.make_reference_forest`).

(a) RandomForestClassifier(50, max_features=min(24, F), n_jobs=1, random_state=s), s = 0..7, on `small` and `grss2013`:
    the eight validation OAs and the accuracy bound the product's own forest is held to,
    min(OA) - max(max(OA) - min(OA), 2 / n_val); for s = 0 the node arrays (leaf rows only where a node is a leaf), the
    labels and probabilities on the validation rows and, for `small`, on every scene row.  The stored forest is served
    through the emulation here, and at most 1 % of the rows may need leaving out (top two probabilities within 1e-12).
(b) DecisionTreeClassifier(max_depth=d, random_state=r), r = 0, 1, 2, on the BIN INDICES (bins from the emulation) of
    forest_cases.TREE_PATH -- `small` with another seed and six classes: on `small` itself the three trees agree only
    to depth 1 -- with d = the largest depth <= DEPTH at which the three trees are identical, i.e. no tie was decided by
    scikit-learn's stream; the JSON says which scene and which d.  One tree is stored, with, per split, the largest bin
    that went left (the product's threshold bin: the lowest bin among equal scores)."""
import json

import numpy as np

from tests import emu_forest, emu_scene  # noqa: F401 -- attach the emulation
from tests import forest_cases as FC
from tests import svm_cases as S
from tests.emu_backend import EmuBackend

DEPTH = 6


def forest_arrays(rf):
    trees = [e.tree_ for e in rf.estimators_]
    off = np.concatenate([[0], np.cumsum([t.node_count for t in trees])]).astype(np.int32)
    cat = lambda f: np.concatenate([f(t) for t in trees])  # noqa: E731
    left = cat(lambda t: t.children_left).astype(np.int32)
    value = cat(lambda t: t.value[:, 0, :])
    leaves = np.flatnonzero(left < 0).astype(np.int32)
    return {"classes": rf.classes_, "n_features": np.int64(rf.n_features_in_),
            "feature": cat(lambda t: t.feature).astype(np.int32), "threshold": cat(lambda t: t.threshold),
            "left": left, "right": cat(lambda t: t.children_right).astype(np.int32), "tree_offsets": off,
            "leaf_nodes": leaves, "leaf_rows": value[leaves]}


def main():
    import sklearn
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.tree import DecisionTreeClassifier
    from hypelcnn_amd.classic.forest import ForestClassifier
    meta = {"sklearn": sklearn.__version__, "cases": {}, "tie_eps": FC.TIE_EPS}
    out = {}
    for case in ("small", "grss2013"):
        X, y, Xv, yv = FC.load(case)
        oas = []
        for s in range(8):
            rf = RandomForestClassifier(FC.SK_TREES, max_features=min(24, X.shape[1]), n_jobs=1, random_state=s).fit(X, y)
            oas.append(float((rf.predict(Xv) == yv).mean()))
            if s == 0:
                first = rf
        spread = max(oas) - min(oas)
        meta["cases"][case] = {"n_train": len(y), "n_val": len(yv), "n_features": X.shape[1], "oa": oas,
                               "oa_bound": min(oas) - max(spread, 2.0 / len(yv))}
        for k, v in forest_arrays(first).items():
            out[f"{case}/rf/{k}"] = v
        served = ForestClassifier.from_arrays(backend=EmuBackend(), **FC.sk_arrays(out, case))
        sets = {"validation": Xv}
        if case == "small":
            sets["scene"] = S.load_scene_rows(FC.CASES[case][0])[0]
        for which, rows in sets.items():
            proba, labels = first.predict_proba(rows), first.predict(rows)
            out[f"{case}/rf/proba_{which}"], out[f"{case}/rf/predict_{which}"] = proba, labels
            FC.check_served_labels(served.predict(rows), proba, labels, f"{case}/{which}")
            print(f"{case}/{which}: max |proba - scikit-learn's| {np.abs(served.predict_proba(rows) - proba).max():.3e}")
        print(case, meta["cases"][case])

    # (b) single tree on the bin indices
    X, y = FC.load_tree_case()
    probe = FC.make("small", EmuBackend(), n_estimators=1, bootstrap=False, max_features=None, max_depth=0).fit(X, y)
    n, f = X.shape
    bins = probe._bins.numpy().reshape(f, probe._ldn)[:, :n].T.copy()
    keys = ("feature", "threshold", "children_left", "children_right", "n_node_samples")
    for depth in range(DEPTH, 0, -1):  # the deepest tree, from DEPTH down, that no random_state changes
        trees = [DecisionTreeClassifier(max_depth=depth, random_state=r).fit(bins, y).tree_ for r in (0, 1, 2)]
        if all(np.array_equal(getattr(t, k), getattr(trees[0], k)) for t in trees[1:] for k in keys):
            break
        print(f"max_depth={depth}: the three trees differ (a tie decided by scikit-learn's stream), trying {depth - 1}")
    else:
        raise AssertionError("no depth at which the three trees agree: change the case's seed")
    t = trees[0]
    left_max = np.full(t.node_count, -1, np.int32)
    path = t.decision_path(bins.astype(np.float32)).toarray().astype(bool)
    for node in np.flatnonzero(t.children_left >= 0):
        rows = path[:, t.children_left[node]]
        left_max[node] = bins[rows, t.feature[node]].max()
    out.update({"small/tree/feature": t.feature.astype(np.int32), "small/tree/left": t.children_left.astype(np.int32),
                "small/tree/right": t.children_right.astype(np.int32), "small/tree/left_max_bin": left_max,
                "small/tree/n_node_samples": t.n_node_samples.astype(np.int32),
                "small/tree/leaf_class": np.argmax(t.value[:, 0, :], 1).astype(np.int32)})
    meta["tree"] = {"case": "small", "path": FC.TREE_PATH, "changed": "seed 1234 -> 2, classes 4 -> 6 (on `small` the "
                    "trees of random_state 0, 1, 2 agree to depth 1 only)", "tree_depth": int(t.max_depth),
                    "max_depth": depth, "max_depth_asked": DEPTH, "random_states": [0, 1, 2], "identical": True,
                    "node_count": int(t.node_count)}
    np.savez_compressed(FC.NPZ_PATH, **out)
    with open(FC.JSON_PATH, "w") as fh:
        json.dump(meta, fh, indent=1)
    print(meta["tree"])


if __name__ == "__main__":
    main()
