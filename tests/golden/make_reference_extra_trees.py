"""Writes tests/golden/extra_trees.npz with scikit-learn (run from the repository root:
`python -m tests.golden.make_reference_extra_trees`).  Recorded data only:

  X_train [400, 30], y_train [400], X_val [800, 30], y_val [800]   a five-class problem, float32 / int64: class
      centres CENTRE_SCALE * N(0, 1) in 30 columns, unit normal noise around them, from
      numpy.random.Generator(PCG64(PROBLEM_SEED)) -- hard enough that a forest of 30 trees is right about half the time,
      so that the validation accuracy has its full binomial spread;
  sk_oa [6]   the validation accuracies of ExtraTreesClassifier(n_estimators=30, max_features=5, random_state=s),
      s = 0..5;
  sklearn     the version that wrote them.

tests/test_extra_trees_emu.py holds the mean accuracy of hypelcnn_amd.classic.forest.ExtraTreesForest(30,
max_features=5) over seeds 0..5 to the recorded mean minus two binomial standard errors of one run."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "extra_trees.npz")
PROBLEM_SEED, CENTRE_SCALE = 2013, 0.34
N_TRAIN, N_VAL, N_COLUMNS, N_CLASSES = 400, 800, 30, 5
TREES, MAX_FEATURES, SEEDS = 30, 5, range(6)


def problem():
    rng = np.random.Generator(np.random.PCG64(PROBLEM_SEED))
    centres = CENTRE_SCALE * rng.standard_normal((N_CLASSES, N_COLUMNS))
    y = rng.integers(0, N_CLASSES, N_TRAIN + N_VAL)
    X = (centres[y] + rng.standard_normal((N_TRAIN + N_VAL, N_COLUMNS))).astype(np.float32)
    return X[:N_TRAIN], y[:N_TRAIN], X[N_TRAIN:], y[N_TRAIN:]


def main():
    import sklearn
    from sklearn.ensemble import ExtraTreesClassifier
    X, y, Xv, yv = problem()
    oa = [float((ExtraTreesClassifier(n_estimators=TREES, max_features=MAX_FEATURES, random_state=s).fit(X, y)
                 .predict(Xv) == yv).mean()) for s in SEEDS]
    np.savez_compressed(PATH, X_train=X, y_train=y, X_val=Xv, y_val=yv, sk_oa=np.array(oa),
                        sklearn=np.array(sklearn.__version__))
    print(f"scikit-learn {sklearn.__version__}: {oa}, mean {np.mean(oa):.4f}; {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
