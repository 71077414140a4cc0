"""Random forest of histogram trees grown and served on the device (reference classify/classic_ml_trainer.py:46,
`RandomForestClassifier(n_estimators=50, max_features=int(2 * sqrt(144)))`; include/hypel.h, hypel_forest_*).

fit: every column is quantised once to at most 256 bins (hypel_forest_bin_edges_f32, hypel_forest_bin_u8); all trees
then grow together, level by level: hypel_forest_split_hist scores every (active node, candidate column) over bin
boundaries with integer class histograms, hypel_forest_split_apply picks the best, writes the node and partitions the
node's rows.  The host reads one counter per level to size the next launch; the loop is bounded by the depth cap.
Randomness is the project's data-side rule -- a seeded host generator, small device tables:
numpy.random.Generator(PCG64(seed)) draws the bootstrap counts, the row permutation of the edge subsample and each
level's candidate table (in active-node order, without replacement per node).  Nothing of scikit-learn's stream is
reproduced.  On purpose, unlike scikit-learn: thresholds lie on bin edges, candidates are not redrawn when all of a node's
are invalid, growth is level-wise (node numbers are breadth-first per tree).

ExtraTreesForest (reference classify/classic_ml_trainer.py:50, `ExtraTreesClassifier`) grows through the same level loop
with another split search: no quantisation, one random cut per node and candidate column on the raw float32 values
(hypel_forest_columns_f32, hypel_forest_split_random, hypel_forest_split_apply_thr); fit() calls the two hooks
_prepare_columns and _split_level for what differs.

predict: hypel_forest_predict_rows walks every tree per row and averages the leaf rows in fp64.  predict_scene walks the
trees straight on the padded scene (hypel_forest_predict_scene) where the data set has one resolution, else it cuts
patches chunk by chunk and uses the row kernel.

Diagnostics, methods of both classes and of a model loaded with from_arrays (what scikit-learn's forests carry as
attributes; none is a constructor argument, get_params() does not change): out_of_bag (hypel_forest_oob_rows: the vote
of the trees whose bootstrap left a training row out -- oob_decision_function_, oob_votes_, oob_score_),
feature_importances (hypel_forest_importances_f64: mean decrease in impurity from node_weight_ and Gini of value_, every
sum in an order the header states) and permutation_importance (hypel_forest_permuted_hits: the columns of a group,
c % group_mod, read from a partner row inside the walk; group_mod = the channel count of flattened patches asks which
band, at every window position together, carries the decision).

There is no CPU fallback: the `backend` argument exists so that the tests can run this file on their numpy emulation
of the same entry points."""
import numpy as np
import torch

from hypelcnn_amd.backend import (FOREST_EDGE_ROWS, FOREST_MAX_CLASSES, FOREST_MAX_DEPTH, FOREST_MAX_EDGES,
                                  FOREST_NODE_DTYPE, Ref)


def _round_up(v, m):
    return (int(v) + m - 1) // m * m


def round_down_f32(thr):
    """The largest float32 not above each float64 threshold: for a float32 x, x <= thr64 holds exactly when x <= that
    value (rounding to nearest can land on the sample above the threshold and flip it)."""
    thr = np.asarray(thr, np.float64)
    t32 = thr.astype(np.float32)
    above = t32.astype(np.float64) > thr
    t32[above] = np.nextafter(t32[above], np.float32(-np.inf))
    return t32


def scene_features(feature, p, wp, cc, cl):
    """Patch feature index -> hypel_forest_predict_scene's (element offset, array) code; leaves (feature < 0) keep 0."""
    f = np.maximum(np.asarray(feature, np.int64), 0)
    c = cc + cl
    pix, ch = f // c, f % c
    pixel = (pix // p) * wp + pix % p
    code = np.where(ch < cc, 2 * (pixel * cc + ch), 2 * (pixel * cl + ch - cc) + 1)
    return np.where(np.asarray(feature) < 0, 0, code).astype(np.int32)


class ForestClassifier:
    """The subset of sklearn.ensemble.RandomForestClassifier the reference uses, on the device.

    Fitted attributes: classes_, n_features_in_, and the flat node arrays over all trees -- tree t owns nodes
    tree_offsets_[t] .. tree_offsets_[t + 1]; feature_ (-1: leaf), threshold_ (float32), left_ / right_ (tree-local
    child numbers like scikit-learn's children_left / children_right, -1: leaf), leaf_ (row of leaf_value_, -1: inner
    node), value_ [n_nodes, n_classes] (class weight fractions), leaf_value_ = value_ of the leaves; after fit also
    threshold_bin_, node_count_ (unique rows), node_weight_ and bootstrap_counts_ [n_trees, n].  After out_of_bag():
    oob_decision_function_, oob_votes_, oob_score_; after feature_importances(): importances_n_used_."""

    def __init__(self, n_estimators=50, max_features=24, bootstrap=True, max_depth=None, n_bins=256, seed=0,
                 backend=None, chunk_rows=None):
        if int(n_estimators) < 1:
            raise ValueError(f"ForestClassifier(n_estimators={n_estimators}): at least one tree")
        if not (max_features is None or max_features == "sqrt" or
                (not isinstance(max_features, str) and int(max_features) >= 1)):
            raise ValueError(f"ForestClassifier(max_features={max_features!r}): a positive int, 'sqrt' or None")
        if not 2 <= int(n_bins) <= FOREST_MAX_EDGES + 1:
            raise ValueError(f"ForestClassifier(n_bins={n_bins}): 2..{FOREST_MAX_EDGES + 1}")
        if max_depth is not None and not 0 <= int(max_depth) <= FOREST_MAX_DEPTH:
            raise ValueError(f"ForestClassifier(max_depth={max_depth}): 0..{FOREST_MAX_DEPTH} (the level loop is bounded)")
        self.n_estimators, self.max_features, self.bootstrap = int(n_estimators), max_features, bool(bootstrap)
        self.max_depth, self.n_bins, self.seed = None if max_depth is None else int(max_depth), int(n_bins), int(seed)
        self._be = backend
        self.chunk_rows = chunk_rows  # rows per serving launch (default: 256 MB of rows)

    def _level_done(self, level, active, n_active, cand, score, best_bin, valid):
        """Called after every level of fit with the level's device tables (a subclass may copy them); nothing here."""

    def _nodes_renumbered(self, model_node):
        """Called once per fit: model_node[device node number] = the node's place in the fitted arrays."""

    def get_params(self):
        return {"bootstrap": self.bootstrap, "max_depth": self.max_depth, "max_features": self.max_features,
                "n_bins": self.n_bins, "n_estimators": self.n_estimators, "seed": self.seed}

    def _backend(self):
        if self._be is None:
            from hypelcnn_amd.backend import HipBackend
            self._be = HipBackend()
        return self._be

    def _rows(self, X):
        """[n, features] (numpy or tensor) -> flat fp32 device tensor [n, features]"""
        be = self._backend()
        t = torch.from_numpy(np.ascontiguousarray(X)) if isinstance(X, np.ndarray) else X
        if t.dim() != 2:
            raise ValueError(f"ForestClassifier: X must be [rows, features], got {tuple(t.shape)}")
        return t.to(be.device).float().contiguous().view(-1), int(t.shape[0]), int(t.shape[1])

    def _resolve_max_features(self, f):
        if self.max_features is None:
            return f
        if self.max_features == "sqrt":
            return max(1, int(np.sqrt(f)))
        return min(int(self.max_features), f)

    def _check_classes(self, classes):
        n_cls = len(classes)
        if n_cls > 255:
            raise ValueError(f"ForestClassifier: {n_cls} classes; labels are written as uint8 (the scene raster of "
                             f"--fullscene is uint8), so at most 255 classes")
        if n_cls > FOREST_MAX_CLASSES:
            raise ValueError(f"ForestClassifier: {n_cls} classes; the class histogram of a node lives in LDS, at most "
                             f"{FOREST_MAX_CLASSES} classes (HYPEL_FOREST_MAX_CLASSES)")

    # ---- fit ---------------------------------------------------------------------------------------------------
    _name = "ForestClassifier"

    def _prepare_columns(self, be, rng, x, n, f, ldn):
        """Once per fit, after the bootstrap draw: the feature-major form of the rows that the split search reads.
        Here: the row permutation of the edge subsample is drawn, then edges and bins."""
        perm = rng.permutation(n).astype(np.int32)
        edges, n_edges = be.empty(f * FOREST_MAX_EDGES), be.zeros(f, torch.int32)
        perm_d = be.upload(perm[:min(n, FOREST_EDGE_ROWS)])
        be.call("forest_bin_edges_f32", Ref(x), f, n, f, Ref(perm_d), self.n_bins, Ref(edges), Ref(n_edges))
        bins = be.zeros(f * ldn, torch.uint8)
        be.call("forest_bin_u8", Ref(x), f, n, f, Ref(edges), Ref(n_edges), Ref(bins), ldn)
        self._edges, self._n_edges, self._bins, self._ldn = edges, n_edges, bins, ldn

    def _split_level(self, be, rng, rows, src, dst, slots, mf, f, score, valid, grown):
        """One level: the split search and its application.  rows = (ldn, y, weight, n, n_classes), slots = (active,
        n_active, cand), grown = the arguments of hypel_forest_split_apply from `level` on.  Returns the level's cut
        table (what _level_done receives beside score and valid)."""
        best_bin = be.zeros(slots[1] * mf, torch.int32)
        be.call("forest_split_hist", Ref(self._bins), *rows, src, *slots, mf, f, score, Ref(best_bin), valid)
        be.call("forest_split_apply", Ref(self._bins), *rows, src, dst, *slots, mf, f, score, Ref(best_bin), valid,
                Ref(self._edges), *grown)
        return best_bin

    def fit(self, X, y):
        be = self._backend()
        y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
        self.classes_, yi = np.unique(y, return_inverse=True)
        self._check_classes(self.classes_)
        n_cls = len(self.classes_)
        x, n, f = self._rows(X)
        if n != len(y):
            raise ValueError(f"ForestClassifier.fit: {n} rows, {len(y)} labels")
        n_trees = self.n_estimators
        mf = self._resolve_max_features(f)
        rng = np.random.Generator(np.random.PCG64(self.seed))
        if self.bootstrap:
            weight = np.stack([np.bincount(rng.integers(0, n, n), minlength=n) for _ in range(n_trees)]).astype(np.int32)
        else:
            weight = np.ones((n_trees, n), np.int32)
        self.bootstrap_counts_ = weight
        ldn = _round_up(n, 4)
        self._prepare_columns(be, rng, x, n, f, ldn)

        # the order array: tree after tree, the tree's unique in-bag rows in ascending order
        in_bag = [np.flatnonzero(weight[t] > 0).astype(np.int32) for t in range(n_trees)]
        uniq = np.array([len(v) for v in in_bag], np.int64)
        starts = np.concatenate([[0], np.cumsum(uniq)[:-1]])
        order = [be.upload(np.concatenate(in_bag)), be.zeros(int(uniq.sum()), torch.int32)]
        capacity = int((2 * uniq - 1).sum())
        y_d, w_d = be.upload(yi.astype(np.int32)), be.upload(weight)
        i32 = {k: be.zeros(capacity, torch.int32)
               for k in ("feature", "thr_bin", "left", "right", "node_tree", "node_count", "node_weight")}
        threshold, value = be.zeros(capacity), be.zeros(capacity * n_cls, torch.float64)
        active = be.upload(np.stack([np.arange(n_trees), starts, uniq, np.arange(n_trees)], 1).astype(np.int32))
        n_active, n_nodes, level = n_trees, n_trees, 0
        cap = FOREST_MAX_DEPTH if self.max_depth is None else self.max_depth
        while n_active > 0 and level <= cap:
            if mf == f:
                cand = np.tile(np.arange(f, dtype=np.int32), (n_active, 1))
            else:
                cand = np.stack([rng.choice(f, mf, replace=False) for _ in range(n_active)]).astype(np.int32)
            cand_d = be.upload(cand)
            score, valid = be.zeros(n_active * mf, torch.float64), be.zeros(n_active * mf, torch.int32)
            split_ws, nxt, counter = (be.zeros(n_active, torch.int32), be.zeros(8 * n_active, torch.int32),
                                      be.zeros(1, torch.int32))
            src, dst = order[level % 2], order[(level + 1) % 2]
            rows = (ldn, Ref(y_d), Ref(w_d), n, n_cls)
            slots = (Ref(active), n_active, Ref(cand_d))
            grown = (level, cap, n_nodes, capacity, Ref(i32["feature"]), Ref(i32["thr_bin"]), Ref(threshold),
                     Ref(i32["left"]), Ref(i32["right"]), Ref(i32["node_tree"]), Ref(i32["node_count"]),
                     Ref(i32["node_weight"]), Ref(value), Ref(split_ws), Ref(nxt), Ref(counter))
            cut = self._split_level(be, rng, rows, Ref(src), Ref(dst), slots, mf, f, Ref(score), Ref(valid), grown)
            n_next = int(counter.cpu()[0])  # (the one small read per level; it also orders the buffers' lifetimes)
            if n_next < 0:
                raise RuntimeError(f"{self._name}.fit: node arrays too small (hypel_forest_split_apply)")
            self._level_done(level, active, n_active, cand, score, cut, valid)
            active, n_active, n_nodes, level = nxt, n_next, n_nodes + n_next, level + 1
        self.n_levels_ = level

        # device numbering is breadth-first over all trees at once; the model keeps each tree's nodes together
        got = {k: v.cpu().numpy()[:n_nodes] for k, v in i32.items()}
        by_tree = np.argsort(got["node_tree"], kind="stable")
        new_id = np.empty(n_nodes, np.int64)
        new_id[by_tree] = np.arange(n_nodes)
        self._nodes_renumbered(new_id)
        offsets = np.concatenate([[0], np.cumsum(np.bincount(got["node_tree"], minlength=n_trees))]).astype(np.int32)
        first = offsets[got["node_tree"][by_tree]]
        child = lambda a: np.where(a[by_tree] >= 0, new_id[np.maximum(a[by_tree], 0)] - first, -1).astype(np.int32)  # noqa: E731
        self.threshold_bin_ = got["thr_bin"][by_tree]
        self.node_count_, self.node_weight_ = got["node_count"][by_tree], got["node_weight"][by_tree]
        self.__dict__.pop("impurity_", None)  # (of an earlier from_arrays: a grown forest's impurity is Gini from value_)
        self._set_model(f, got["feature"][by_tree], threshold.cpu().numpy()[:n_nodes][by_tree], child(got["left"]),
                        child(got["right"]), offsets,
                        value.cpu().numpy()[:n_nodes * n_cls].reshape(n_nodes, n_cls)[by_tree])
        return self

    # ---- the served model ----------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, classes, n_features, feature, threshold, left, right, tree_offsets, value, backend=None,
                    node_weight=None, impurity=None):
        """A served model from flat node arrays (see the class docstring; scikit-learn's tree_.feature, .threshold,
        .children_left, .children_right and .value[:, 0, :] of every estimator, concatenated).  float64 thresholds are
        rounded DOWN to float32.  node_weight and impurity (optional; tree_.weighted_n_node_samples and tree_.impurity)
        are what feature_importances() needs: without impurity it is Gini from `value`."""
        self = cls(n_estimators=len(tree_offsets) - 1, backend=backend)
        self.classes_ = np.asarray(classes)
        self._check_classes(self.classes_)
        self._set_model(int(n_features), np.asarray(feature), np.asarray(threshold), np.asarray(left), np.asarray(right),
                        np.asarray(tree_offsets), np.asarray(value, np.float64))
        for name, a in (("node_weight_", node_weight), ("impurity_", impurity)):
            if a is not None:
                a = np.ascontiguousarray(a, np.float64).reshape(-1)
                if len(a) != len(self.feature_):
                    raise ValueError(f"ForestClassifier.from_arrays: {name[:-1]} has {len(a)} entries, the model "
                                     f"{len(self.feature_)} nodes")
                setattr(self, name, a)
        return self

    def _set_model(self, n_features, feature, threshold, left, right, tree_offsets, value):
        be = self._backend()
        off = np.asarray(tree_offsets, np.int64)
        n_nodes, n_cls = len(feature), len(self.classes_)
        if len(off) < 2 or off[0] != 0 or off[-1] != n_nodes or (np.diff(off) < 1).any():
            raise ValueError("ForestClassifier: tree_offsets must run from 0 to the node count, one node per tree at least")
        if not (len(threshold) == len(left) == len(right) == n_nodes and value.shape == (n_nodes, n_cls)):
            raise ValueError("ForestClassifier: node arrays of different lengths")
        left, right = left.astype(np.int64), right.astype(np.int64)
        is_leaf = left < 0
        feature = np.where(is_leaf, -1, feature).astype(np.int32)
        local = np.arange(n_nodes) - np.repeat(off[:-1], np.diff(off))
        size = np.repeat(np.diff(off), np.diff(off))
        inner = ~is_leaf
        ok = ((left[inner] > local[inner]) & (left[inner] < size[inner]) & (right[inner] > local[inner]) &
              (right[inner] < size[inner]) & (feature[inner] >= 0) & (feature[inner] < n_features))
        if not ok.all() or (right[is_leaf] >= 0).any():
            raise ValueError("ForestClassifier: a child must lie after its parent inside its tree, a split feature inside "
                             "the row")
        thr = round_down_f32(np.where(is_leaf, 0.0, threshold)) if threshold.dtype != np.float32 else \
            np.where(is_leaf, np.float32(0), threshold).astype(np.float32)
        self.n_features_in_ = n_features
        self.n_estimators = len(off) - 1
        self.feature_, self.threshold_, self.left_, self.right_ = feature, thr, left.astype(np.int32), right.astype(np.int32)
        self.tree_offsets_, self.value_ = off.astype(np.int32), value
        self.leaf_ = np.where(is_leaf, np.cumsum(is_leaf) - 1, -1).astype(np.int32)
        self.leaf_value_ = np.ascontiguousarray(value[is_leaf])
        base = np.repeat(off[:-1], np.diff(off))
        self._abs = [np.where(is_leaf, -1, a + base).astype(np.int32) for a in (left, right)]
        self._dev = {"tree_off": be.upload(self.tree_offsets_[:-1]), "nodes": be.upload(self._node_records(feature)),
                     "leaf_value": be.upload(self.leaf_value_)}
        self._scene_key, self._scene_nodes = None, None
        self._labels_u8 = None
        if self.classes_.dtype.kind in "iu" and self.classes_.min() >= 0 and self.classes_.max() <= 255:
            self._labels_u8 = be.upload(self.classes_.astype(np.uint8))

    def arrays(self):
        """The arguments of from_arrays that describe the nodes."""
        return {"feature": self.feature_, "threshold": self.threshold_, "left": self.left_, "right": self.right_,
                "tree_offsets": self.tree_offsets_, "value": self.value_}

    def _node_records(self, feature):
        """hypel_forest_node_t of every node; `feature` is what an inner node reads (a column, or a scene code)"""
        rec = np.zeros(len(self.feature_), FOREST_NODE_DTYPE)
        inner = self.leaf_ < 0
        rec["feature"], rec["threshold"] = np.where(inner, feature, 0), np.where(inner, self.threshold_, 0)
        rec["left"], rec["right"] = np.where(inner, self._abs[0], -1 - self.leaf_), np.where(inner, self._abs[1], 0)
        return rec

    def _model_args(self, nodes):
        d = self._dev
        return (Ref(d["tree_off"]), self.n_estimators, Ref(nodes), len(self.feature_), Ref(d["leaf_value"]),
                len(self.leaf_value_), len(self.classes_))

    def _fitted(self):
        if not hasattr(self, "feature_"):
            raise RuntimeError("ForestClassifier: fit first")

    # ---- predict -----------------------------------------------------------------------------------------------
    def _chunk(self, n):
        if self.chunk_rows:
            return max(1, min(int(self.chunk_rows), n))
        return max(1, min(n, (1 << 28) // (4 * self.n_features_in_)))

    def _chunks(self, n, produce):
        """The chunked serving loop: yields (r0, x, m, f), where x, m, f = produce(r0, r1) are a chunk's rows on the
        device, their number and their feature count; synchronises after each chunk (x dies there)."""
        step = self._chunk(n)
        for r0 in range(0, n, step):
            yield (r0, *produce(r0, min(n, r0 + step)))
            self._be.synchronize()

    def _check_features(self, got, where):
        if got != self.n_features_in_:
            raise ValueError(f"{where}: X has {got} features, the model was fitted on {self.n_features_in_}")

    def _run(self, X, want_proba):
        be = self._backend()
        self._fitted()
        n = X.shape[0]
        self._check_features(X.shape[1], "ForestClassifier")
        n_cls = len(self.classes_)
        idx = be.zeros(_round_up(n, 4), torch.uint8)
        proba = be.zeros(n * n_cls, torch.float64) if want_proba else None
        for r0, x, m, f in self._chunks(n, lambda r0, r1: self._rows(X[r0:r1])):
            be.call("forest_predict_rows", Ref(x), f, m, f, *self._model_args(self._dev["nodes"]), None, None,
                    Ref(idx, r0), 0, None if proba is None else Ref(proba, r0 * n_cls))
        return idx.cpu().numpy()[:n], None if proba is None else proba.cpu().numpy().reshape(n, n_cls)

    def predict(self, X):
        return self.classes_[self._run(X, False)[0]]

    def predict_proba(self, X):
        return self._run(X, True)[1]

    # ---- diagnostics -------------------------------------------------------------------------------------------
    def _class_index(self, y, n, where):
        """labels -> int32 indices into classes_ (-1: a label the model does not know; it never counts as a hit)"""
        y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
        if len(y) != n:
            raise ValueError(f"{self._name}.{where}: {n} rows, {len(y)} labels")
        at = np.minimum(np.searchsorted(self.classes_, y), len(self.classes_) - 1)
        return y, np.where(self.classes_[at] == y, at, -1).astype(np.int32)

    def out_of_bag(self, X, y, in_bag_counts=None):
        """scikit-learn's oob_score=True on the device (hypel_forest_oob_rows): every row of the training matrix X is
        voted on by the trees whose bootstrap left it out.  Sets oob_decision_function_ [n, n_classes] (the mean leaf
        row of the voting trees; zeros where no tree votes), oob_votes_ [n] and oob_score_ (the accuracy of the
        first-maximum labels, computed on the host) and returns the score.  in_bag_counts [n_trees, n] defaults to the
        bootstrap_counts_ of fit(); a model from from_arrays passes its own (scikit-learn: the bincount of
        _generate_sample_indices per estimator)."""
        be = self._backend()
        self._fitted()
        counts = getattr(self, "bootstrap_counts_", None) if in_bag_counts is None else np.asarray(in_bag_counts)
        if in_bag_counts is None and not self.bootstrap:
            raise ValueError("Out of bag estimation only available if bootstrap=True")
        if counts is None:
            raise ValueError(f"{self._name}.out_of_bag: a model from from_arrays has no bootstrap_counts_: pass "
                             f"in_bag_counts [n_trees, n]")
        n, n_cls, n_trees = X.shape[0], len(self.classes_), self.n_estimators
        self._check_features(X.shape[1], f"{self._name}.out_of_bag")
        if counts.shape != (n_trees, n):
            raise ValueError(f"{self._name}.out_of_bag: in-bag counts of shape {counts.shape}, X has {n} rows and the "
                             f"forest {n_trees} trees: out-of-bag rows are rows of the training matrix")
        y, _ = self._class_index(y, n, "out_of_bag")
        w_d = be.upload(np.ascontiguousarray(counts, np.int32))
        idx, votes = be.zeros(_round_up(n, 4), torch.uint8), be.zeros(n, torch.int32)
        proba = be.zeros(n * n_cls, torch.float64)
        for r0, x, m, f in self._chunks(n, lambda r0, r1: self._rows(X[r0:r1])):
            be.call("forest_oob_rows", Ref(x), f, m, f, *self._model_args(self._dev["nodes"]), None, Ref(w_d, r0), n,
                    Ref(idx, r0), Ref(proba, r0 * n_cls), Ref(votes, r0))
        self.oob_decision_function_ = proba.cpu().numpy().reshape(n, n_cls)
        self.oob_votes_ = votes.cpu().numpy()
        self.oob_score_ = float(np.mean(self.classes_[idx.cpu().numpy()[:n]] == y))
        if (self.oob_votes_ == 0).any():
            import warnings
            warnings.warn(f"{self._name}.out_of_bag: {int((self.oob_votes_ == 0).sum())} of {n} rows are in every tree's "
                          f"bag (too few trees): their row of oob_decision_function_ is zeros and counts as class "
                          f"{self.classes_[0]!r}")
        return self.oob_score_

    def feature_importances(self, per_tree=False):
        """scikit-learn's feature_importances_ (mean decrease in impurity) on the device
        (hypel_forest_importances_f64): node_weight_ of the fit and Gini from value_, or the node_weight / impurity
        given to from_arrays.  Returns [n_features] (sum 1, or all zeros where no tree has a split), with
        per_tree=True the pair (that, [n_trees, n_features] normalised per tree); importances_n_used_ = the trees with
        more than one node."""
        be = self._backend()
        self._fitted()
        weight = getattr(self, "node_weight_", None)
        if weight is None:
            raise ValueError(f"{self._name}.feature_importances: the model was loaded without node_weight "
                             f"(from_arrays(..., node_weight=tree_.weighted_n_node_samples))")
        impurity = getattr(self, "impurity_", None)
        f, n_trees, n_nodes = self.n_features_in_, self.n_estimators, len(self.feature_)
        rows, imp, used = be.zeros(n_trees * f, torch.float64), be.zeros(f, torch.float64), be.zeros(1, torch.int32)
        w_d = be.upload(np.ascontiguousarray(weight, np.float64))
        v_d = be.upload(np.ascontiguousarray(self.value_, np.float64))
        i_d = None if impurity is None else be.upload(impurity)
        be.call("forest_importances_f64", Ref(self._dev["nodes"]), n_nodes, Ref(self._dev["tree_off"]), n_trees, Ref(v_d),
                len(self.classes_), Ref(w_d), None if i_d is None else Ref(i_d), f, Ref(rows), Ref(imp), Ref(used))
        be.synchronize()
        self.importances_n_used_ = int(used.cpu()[0])
        out = imp.cpu().numpy()
        return (out, rows.cpu().numpy().reshape(n_trees, f)) if per_tree else out

    def permutation_importance(self, X, y, n_repeats=5, group_mod=None, seed=0, groups_per_launch=None):
        """Grouped permutation importance on the device (hypel_forest_permuted_hits): column c belongs to group
        c % group_mod (None: every column its own group; the channel count of flattened patches: one band at every
        window position).  Per repeat ONE permutation of the rows is drawn, numpy.random.Generator(PCG64(seed)),
        rng.permutation(n), and shared by all groups; a group's columns are read from the partner row, the others from
        the row itself, inside the walk -- no permuted copy of X is made, but all of X is on the device at once.
        Returns a dict: baseline (accuracy of predict), hits int64 [groups, repeats] (rows still classified as y),
        importances = baseline - hits / n, importances_mean and importances_std (over the repeats, ddof 0).  This is
        not sklearn.inspection.permutation_importance's random stream (it redraws per column)."""
        be = self._backend()
        self._fitted()
        x, n, f = self._rows(X)
        self._check_features(f, f"{self._name}.permutation_importance")
        group_mod = f if group_mod is None else int(group_mod)
        n_repeats = int(n_repeats)
        if group_mod < 1 or n_repeats < 1:
            raise ValueError(f"{self._name}.permutation_importance: group_mod={group_mod}, n_repeats={n_repeats}: both >= 1")
        y, yi = self._class_index(y, n, "permutation_importance")
        baseline = float(np.mean(self.predict(X) == y))
        rng = np.random.Generator(np.random.PCG64(seed))
        partner = be.upload(np.stack([rng.permutation(n) for _ in range(n_repeats)]).astype(np.int32))
        y_d = be.upload(yi)
        row_blocks = (n + 63) // 64
        # groups per launch: the grid below 2^24 blocks (far inside the entry point's 2^31 - 1), the hit table with it
        step = groups_per_launch or max(1, (1 << 24) // (row_blocks * n_repeats))
        hits = np.zeros((group_mod, n_repeats), np.int64)
        for g0 in range(0, group_mod, step):
            g = min(step, group_mod - g0)
            part = be.zeros(g * n_repeats, torch.int32)
            be.call("forest_permuted_hits", Ref(x), f, n, f, *self._model_args(self._dev["nodes"]), Ref(y_d),
                    Ref(partner), n_repeats, group_mod, g0, g, Ref(part))
            hits[g0:g0 + g] = part.cpu().numpy().reshape(g, n_repeats)
        imp = baseline - hits / float(n)
        return {"baseline": baseline, "hits": hits, "importances": imp, "importances_mean": imp.mean(1),
                "importances_std": imp.std(1)}

    def predict_scene(self, arrays, raster, raster_w, direct=None):
        """Whole-scene path: `arrays` is a common_nn_ops.SceneArrays fed with the padded scene and the (x, y) targets,
        `raster` a flat uint8 device tensor that receives classes_[winner] at y * raster_w + x.  direct=None takes
        hypel_forest_predict_scene where the data set is the single-resolution kind hypel_gather_patches_f32 serves and
        the chunked gather + hypel_forest_predict_rows otherwise (GRSS2018's 2x layout, multi-scene sets); False forces
        the gather path."""
        be = self._backend()
        self._fitted()
        if self._labels_u8 is None:
            raise ValueError("ForestClassifier.predict_scene: class labels must be integers in 0..255 for the uint8 raster")
        n = len(arrays)
        p, _, c = arrays.shape
        if p * p * c != self.n_features_in_:
            raise ValueError(f"ForestClassifier.predict_scene: patches of {p * p * c} features, the model has "
                             f"{self.n_features_in_}")
        single = arrays.scenes is None and arrays.casi_scale == 1
        if direct is None:
            direct = single
        if direct:
            if not single:
                raise ValueError("ForestClassifier.predict_scene(direct=True): a single-resolution, single-scene data set")
            hp, wp, cc = (int(v) for v in arrays.casi.shape)
            cl = 0 if arrays.lidar is None else int(arrays.lidar.shape[2])
            if self._scene_key != (p, wp, cc, cl):  # translated once per scene geometry
                self._scene_nodes = be.upload(self._node_records(scene_features(self.feature_, p, wp, cc, cl)))
                self._scene_key = (p, wp, cc, cl)
            be.call("forest_predict_scene", Ref(arrays.casi.reshape(-1)),
                    None if arrays.lidar is None else Ref(arrays.lidar.reshape(-1)), hp, wp, cc, cl,
                    Ref(arrays.points.reshape(-1)), n, p, *self._model_args(self._scene_nodes), Ref(self._labels_u8),
                    Ref(raster), int(raster_w))
            be.synchronize()
            return

        def gathered(r0, r1):
            return arrays.gather(torch.arange(r0, r1, device=be.device)), r1 - r0, self.n_features_in_
        for _, (patches, pts), m, f in self._chunks(n, gathered):
            be.call("forest_predict_rows", Ref(patches.reshape(-1)), f, m, f, *self._model_args(self._dev["nodes"]),
                    Ref(self._labels_u8), Ref(pts.reshape(-1)), Ref(raster), int(raster_w), None)


class ExtraTreesForest(ForestClassifier):
    """The subset of sklearn.ensemble.ExtraTreesClassifier the reference names (classify/classic_ml_trainer.py:50), on
    the device: per node and candidate column ONE cut, drawn uniformly inside the range of the node's raw float32
    values (hypel_forest_split_random), the best-scoring candidate taken (hypel_forest_split_apply_thr).  No column is
    quantised, so there is no n_bins and threshold_bin_ is all -1; every other fitted attribute, from_arrays, arrays()
    and the three serving calls are ForestClassifier's.

    Random stream, numpy.random.Generator(PCG64(seed)) on the host, in this order: with bootstrap=True the bootstrap
    counts, tree after tree, as ForestClassifier draws them (bootstrap=False, the default as in scikit-learn: weights
    all one and no draw); then per level the candidate table exactly as ForestClassifier draws it (max_features == the
    column count: no draw; else one rng.choice(f, max_features, replace=False) per active node, in active-node order)
    followed by u = rng.random((n_active, max_features), dtype=float32).  There is no edge permutation.

    On purpose, unlike scikit-learn: its random stream is not reproduced; candidates are not redrawn when all of a
    node's are constant (the node becomes an impure leaf); growth is level-wise; a node at the depth cap (max_depth, at
    most HYPEL_FOREST_MAX_DEPTH) is an impure leaf -- n_levels_ (the number of levels grown) shows when the cap was
    reached."""
    _name = "ExtraTreesForest"

    def __init__(self, n_estimators=50, max_features=24, bootstrap=False, max_depth=None, seed=0, backend=None,
                 chunk_rows=None):
        super().__init__(n_estimators=n_estimators, max_features=max_features, bootstrap=bootstrap, max_depth=max_depth,
                         seed=seed, backend=backend, chunk_rows=chunk_rows)

    def get_params(self):
        p = super().get_params()
        del p["n_bins"]
        return p

    def _prepare_columns(self, be, rng, x, n, f, ldn):
        xt = be.zeros(f * ldn)
        be.call("forest_columns_f32", Ref(x), f, n, f, Ref(xt), ldn)
        self._xt, self._ldn = xt, ldn

    def _split_level(self, be, rng, rows, src, dst, slots, mf, f, score, valid, grown):
        n_active = slots[1]
        u = be.upload(rng.random((n_active, mf), dtype=np.float32))
        thr = be.zeros(n_active * mf)
        be.call("forest_split_random", Ref(self._xt), *rows, src, *slots, Ref(u), mf, f, score, Ref(thr), valid)
        be.call("forest_split_apply_thr", Ref(self._xt), *rows, src, dst, *slots, mf, f, score, Ref(thr), valid, *grown)
        return thr
