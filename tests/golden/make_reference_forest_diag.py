"""Writes tests/golden/reference_forest_diag.npz with scikit-learn (run from the repository root:
`python -m tests.golden.make_reference_forest_diag`).

RandomForestClassifier(20, max_features=4, oob_score=True, random_state=0) on a 300-row, 12-column, 5-class float32
problem (drawn here, stored): the node arrays of every tree with weighted_n_node_samples and impurity, the per-tree in-bag
counts (the bincount of _generate_sample_indices, what scikit-learn's own out-of-bag pass uses), and what the forest
diagnostics are compared with: oob_decision_function_, oob_score_, feature_importances_ of the forest and of every
tree.  No row may lack an out-of-bag vote."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_forest_diag.npz")
N, F, C = 300, 12, 5


def problem():
    rng = np.random.default_rng(2013)
    centres = rng.standard_normal((C, F)) * 1.5
    y = rng.integers(0, C, N)
    X = (centres[y] + rng.standard_normal((N, F)) * 1.2).astype(np.float32)
    X[:, 8:] = rng.standard_normal((N, F - 8)).astype(np.float32)  # four columns without signal
    return X, (10 + 3 * y).astype(np.int64)


def main():
    import sklearn
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.ensemble._forest import _generate_sample_indices
    X, y = problem()
    rf = RandomForestClassifier(20, max_features=4, oob_score=True, random_state=0).fit(X, y)
    trees = [e.tree_ for e in rf.estimators_]
    cat = lambda f: np.concatenate([f(t) for t in trees])  # noqa: E731
    in_bag = np.stack([np.bincount(_generate_sample_indices(e.random_state, N, N), minlength=N)
                       for e in rf.estimators_]).astype(np.int32)
    assert ((in_bag == 0).sum(0) > 0).all(), "a row without an out-of-bag vote: change the seed"
    out = {"X": X, "y": y, "classes": rf.classes_, "n_features": np.int64(F),
           "feature": cat(lambda t: t.feature).astype(np.int32), "threshold": cat(lambda t: t.threshold),
           "left": cat(lambda t: t.children_left).astype(np.int32),
           "right": cat(lambda t: t.children_right).astype(np.int32),
           "tree_offsets": np.concatenate([[0], np.cumsum([t.node_count for t in trees])]).astype(np.int32),
           "value": cat(lambda t: t.value[:, 0, :]), "node_weight": cat(lambda t: t.weighted_n_node_samples),
           "impurity": cat(lambda t: t.impurity), "in_bag": in_bag,
           "oob_decision_function": rf.oob_decision_function_, "oob_score": np.float64(rf.oob_score_),
           "feature_importances": rf.feature_importances_,
           "tree_importances": np.stack([e.feature_importances_ for e in rf.estimators_]),
           "sklearn": np.array(sklearn.__version__)}
    np.savez_compressed(PATH, **out)
    print(f"{PATH}: {os.path.getsize(PATH)} bytes, {len(out['feature'])} nodes, oob_score {rf.oob_score_:.4f}")


if __name__ == "__main__":
    main()
