"""Classic-ML baseline (reference classify/classic_ml_trainer.py:20-157): a kernel SVC, a random forest or an extra-trees forest on flattened
patches, trained and served on the device by hypelcnn_amd.classic.svc.SVC / hypelcnn_amd.classic.forest.ForestClassifier,
with the reference's flow, flag names and output files --
`confusion_matrix_<loader>_run<i>.csv`, `metrics_<loader>_run<i>.txt` (OA,AA,KAPPA) and `params_<loader>_run<i>.json`
under --base_log_path, next to which utilities/latex_table_from_conf_set*.py expects the CNN's.

Differences from the reference, all on purpose:
 - the estimator, which the reference picks by editing comments (:46-50), is a flag: --estimator svc_rbf (its GRSS2013
   line :49, gamma 1e-09, C 10000; --svc_gamma / --svc_c / --svc_tol) or svc_poly (its :48, degree 1, gamma "scale");
 - the reference's live line (:46, RandomForestClassifier(n_estimators=50, max_features=int(2 * sqrt(144)))) is
   --estimator forest: a forest of histogram trees grown and served on the device (--forest_trees 50,
   --forest_max_features 24, --forest_bins 256, --forest_seed 0 + the run index), with a random stream of its own,
   thresholds on bin edges, no candidate redraw and level-wise growth.  scikit-learn's estimator itself,
   asked for by name (RandomForestClassifier, random_forest, rf, ExtraTreesClassifier), stays refused: its result is
   its random stream's, which this project does not reproduce;
 - the reference's commented line :50 (ExtraTreesClassifier) is --estimator extra_trees: random-threshold trees on the
   raw float32 values (hypelcnn_amd.classic.forest.ExtraTreesForest), under the same three flags --forest_trees,
   --forest_max_features and --forest_seed (--forest_bins is ignored: nothing is quantised); no bootstrap, as in
   scikit-learn;
 - what scikit-learn's forests carry as attributes is asked for by NEW flags, valid with forest and extra_trees only and
   computed on the device: --forest_oob (oob_score_ on the training rows; extra_trees, built without
   bootstrap, answers with scikit-learn's ValueError), --forest_importances (feature_importances_) and
   --forest_permutation_repeats N (a permutation importance per band on the validation rows, one band at every window
   position permuted together).  They write forest_diagnostics_<loader>_run<i>.json, band_importance_<loader>_run<i>.csv
   and feature_importance_<loader>_run<i>.npy after the reference's three files, which do not change;
 - the reference's search (:126-136, GridSearchCV(SVC(), C x gamma) over StratifiedShuffleSplit(2, 0.1, 42)) runs on
   the device under a NEW flag, --svc_grid (hypelcnn_amd.classic.model_selection): after the baseline fit and its three
   files it searches the flattened training data, prints the reference's line and writes svc_grid_<loader>_run<i>.json;
   --svc_grid_c / --svc_grid_gamma take lo:hi:n decades (defaults: the reference's -2:10:13 and -9:3:13),
   --svc_grid_refit refits on the best cell and serves --fullscene from that estimator.  --hyperparamopt itself stays
   refused: its contract in the reference is scikit-learn's own GridSearchCV object, which this project does not return;
 - what every published SVM / forest baseline of these scenes also reports, a PCA over the band axis in front of the
   estimator, is two NEW flags, valid with all four estimators and every other flag: --pca_components K (a count, or a
   fraction below 1: the share of the variance to keep; 0, the default: off) and --pca_whiten.  The PCA
   (hypelcnn_amd.classic.decomposition.BandPCA) is fitted once per process on the interior of the loader's
   scene, before the episodes; every episode's patches are projected pixel by pixel with the LiDAR channels passed
   through, --fullscene is served from the projected scene, and the band axis of the forest diagnostics then means
   components.  pca_<loader>.json (n_components, n_samples, bands, whiten, explained_variance,
   explained_variance_ratio) and pca_<loader>.npz (mean_, components_, explained_variance_) are written beside the
   result files.  With --pca_components 0 nothing changes: not a launch, not a file, not a byte of output;
 - the step the same baselines put AFTER the PCA, the extended morphological profile ("PCA -> EMP -> SVM / RF"), is
   four NEW flags, valid with all four estimators and every other flag: --emp_radii 2,4,6,8 (absent or empty: off),
   --emp_shape disk|square, --emp_plain (plain openings and closings instead of those by reconstruction) and --emp_lidar
   true|false (default true: the LiDAR channels are profiled as further bases).  The profile
   (hypelcnn_amd.classic.morphology.MorphologicalProfile) is computed once per process on the interior of the
   loader's scene, after the PCA if there is one.  A profile is no per-pixel function, so patches are not transformed:
   the loader's load_samples(0.1, 0) targets -- the call InMemoryImporter.read_data_set makes -- are cut from the profiled
   scene on the device, --fullscene classifies that same scene, and the band axis of the forest diagnostics then means
   profile channels.  emp_<loader>.json (radii, shape, by_reconstruction, include_lidar, bases, channels, sweeps per
   level, seconds) is written beside the result files.  Without --emp_radii nothing changes;
 - --fullscene writes result_raw.tif / result_colorized.tif under --output_path, not the reference's hard-wired ".."
   (:111); patches are cut on the device (hypel_gather_patches_f32) and predicted in chunks sized from free memory,
   independent of --batch_size; the forest walks its trees straight on the padded scene where the data set has one
   resolution (hypel_forest_predict_scene);
 - OA / AA / kappa come from the confusion matrix on the host (sklearn.metrics' definitions, :56-59)."""
import argparse
import json
import os
import sys
import time
import types

import numpy

from hypelcnn_amd.common.cmd_parser import add_parse_cmds_for_loaders, add_parse_cmds_for_loggers, \
    add_parse_cmds_for_trainers, type_ensure_strtobool
from hypelcnn_amd.common.common_nn_ops import SceneArrays, create_colored_image, get_loader_from_name
from hypelcnn_amd.common.tiff_io import imwrite
from hypelcnn_amd.importer.InMemoryImporter import InMemoryImporter

ESTIMATORS = ("svc_rbf", "svc_poly", "forest", "extra_trees")


def add_parse_cmds_for_app(parser):
    parser.add_argument("--hyperparamopt", nargs="?", const=True, type=type_ensure_strtobool, default=False,
                        help="If true, performs hyper parameter optimization.")
    parser.add_argument("--fullscene", nargs="?", const=True, type=type_ensure_strtobool, default=False,
                        help="If true, performs full scene classification.")
    parser.add_argument("--split_count", nargs="?", type=int, default=1, help="Split count")
    parser.add_argument("--estimator", nargs="?", type=str, default="svc_rbf",
                        help="svc_rbf (reference :49), svc_poly (reference :48), forest (reference :46) or extra_trees "
                             "(reference :50)")
    parser.add_argument("--svc_gamma", nargs="?", type=float, default=1e-09, help="RBF gamma (svc_rbf)")
    parser.add_argument("--svc_c", nargs="?", type=float, default=None, help="C (default: 10000 svc_rbf, 1 svc_poly)")
    parser.add_argument("--svc_tol", nargs="?", type=float, default=1e-3, help="Stopping tolerance of the solver")
    parser.add_argument("--forest_trees", nargs="?", type=int, default=50, help="Trees of the forest (forest, extra_trees)")
    parser.add_argument("--forest_max_features", nargs="?", type=int, default=24,
                        help="Candidate features per node (forest, extra_trees; the reference's int(2 * sqrt(144)))")
    parser.add_argument("--forest_bins", nargs="?", type=int, default=256, help="Bins per feature, 2..256 (forest; ignored by extra_trees, which quantises nothing)")
    parser.add_argument("--forest_seed", nargs="?", type=int, default=0,
                        help="Seed of the forest's random stream; episode i of --split_count uses seed + i")
    parser.add_argument("--forest_oob", nargs="?", const=True, type=type_ensure_strtobool, default=False,
                        help="If true, scores the forest out of bag on the training rows (forest; extra_trees is built "
                             "without bootstrap and refuses).")
    parser.add_argument("--forest_importances", nargs="?", const=True, type=type_ensure_strtobool, default=False,
                        help="If true, writes the impurity importances per feature and per band (forest, extra_trees).")
    parser.add_argument("--forest_permutation_repeats", nargs="?", type=int, default=0,
                        help="Repeats of the per-band permutation importance on the validation rows; 0: off (forest, "
                             "extra_trees)")
    parser.add_argument("--svc_grid", nargs="?", const=True, type=type_ensure_strtobool, default=False,
                        help="If true, searches C x gamma on the device after the baseline fit (reference :126-136).")
    # (a decade range such as -2:10:13 starts with '-' and is no number, so argparse would take it for an option:
    #  main() hands these two flags over as --flag=value, see join_decade_values; a further flag of this form belongs there)
    parser.add_argument("--svc_grid_c", type=str, default="-2:10:13", help="C decades lo:hi:n")
    parser.add_argument("--svc_grid_gamma", type=str, default="-9:3:13", help="gamma decades lo:hi:n")
    parser.add_argument("--svc_grid_refit", nargs="?", const=True, type=type_ensure_strtobool, default=False,
                        help="If true, refits on the best cell; --fullscene then uses that estimator.")
    parser.add_argument("--pca_components", nargs="?", type=parse_pca_components, default=0,
                        help="Band PCA in front of the estimator: components kept (an integer), or the share of the "
                             "variance to keep (a fraction below 1); 0: off")
    parser.add_argument("--pca_whiten", nargs="?", const=True, type=type_ensure_strtobool, default=False,
                        help="If true, scales the kept components to unit variance (with --pca_components).")
    parser.add_argument("--emp_radii", nargs="?", const=(), type=parse_emp_radii, default=(),
                        help="Extended morphological profile behind the PCA (if any): the radii of the structuring "
                             "elements, strictly increasing, e.g. 2,4,6,8; absent or empty: off")
    parser.add_argument("--emp_shape", nargs="?", type=str, default="disk", choices=("disk", "square"),
                        help="Structuring element of the profile (with --emp_radii)")
    parser.add_argument("--emp_plain", nargs="?", const=True, type=type_ensure_strtobool, default=False,
                        help="If true, plain openings and closings instead of those by reconstruction (with --emp_radii).")
    parser.add_argument("--emp_lidar", nargs="?", const=True, type=type_ensure_strtobool, default=True,
                        help="If true (the default), the LiDAR channels are profiled as further bases; if false they pass "
                             "through untouched (with --emp_radii).")


def parse_emp_radii(text):
    """'' (off) or integers separated by commas; the range and the order are MorphologicalProfile's to check"""
    try:
        return tuple(int(part) for part in text.split(",") if part.strip())
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: radii as integers separated by commas, e.g. 2,4,6,8") from None


def parse_pca_components(text):
    """'0' (off), an integer >= 1 (components) or a fraction in (0, 1) (share of the variance)"""
    try:
        value = int(text)
    except ValueError:
        try:
            value = float(text)
        except ValueError:
            value = -1.0
        if not 0.0 < value < 1.0:
            raise argparse.ArgumentTypeError(f"{text!r}: 0, a count of components or a fraction below 1") from None
    if value < 0:
        raise argparse.ArgumentTypeError(f"{text!r}: 0, a count of components or a fraction below 1")
    return value


def create_estimator(flags, backend=None, run_index=0):
    from hypelcnn_amd.classic.svc import SVC
    name = flags.estimator
    if name in ("random_forest", "rf", "RandomForestClassifier", "ExtraTreesClassifier"):
        raise NotImplementedError(
            f"--estimator {name}: scikit-learn's RandomForestClassifier (reference classic_ml_trainer.py:46) is not built: "
            f"its result is that of scikit-learn's random stream, which is not reproduced here; --estimator forest grows "
            f"the same kind of forest on the device with a seeded stream of its own (--estimator extra_trees: the "
            f"random-threshold kind of ExtraTreesClassifier); use one of {ESTIMATORS}")
    if name == "forest":
        from hypelcnn_amd.classic.forest import ForestClassifier
        return ForestClassifier(n_estimators=flags.forest_trees, max_features=flags.forest_max_features,
                                n_bins=flags.forest_bins, seed=flags.forest_seed + run_index, backend=backend)
    if name == "extra_trees":
        from hypelcnn_amd.classic.forest import ExtraTreesForest
        return ExtraTreesForest(n_estimators=flags.forest_trees, max_features=flags.forest_max_features,
                                seed=flags.forest_seed + run_index, backend=backend)
    if name == "svc_rbf":
        return SVC(kernel="rbf", gamma=flags.svc_gamma, C=10000.0 if flags.svc_c is None else flags.svc_c,
                   tol=flags.svc_tol, backend=backend)
    if name == "svc_poly":
        return SVC(kernel="poly", degree=1, gamma="scale", C=1.0 if flags.svc_c is None else flags.svc_c,
                   tol=flags.svc_tol, backend=backend)
    raise ValueError(f"--estimator {name}: one of {ESTIMATORS}")


def flatten_data(data):
    return numpy.reshape(data, [data.shape[0], data.shape[1] * data.shape[2] * data.shape[3]])


def confusion_matrix(labels, predicted):
    """sklearn.metrics.confusion_matrix: rows = truth, columns = prediction, over the sorted labels seen in either."""
    labels, predicted = numpy.asarray(labels).astype(numpy.int64), numpy.asarray(predicted).astype(numpy.int64)
    seen = numpy.unique(numpy.concatenate([labels, predicted]))
    index = numpy.searchsorted(seen, numpy.arange(seen.max() + 1))
    cm = numpy.zeros((len(seen), len(seen)), numpy.int64)
    numpy.add.at(cm, (index[labels], index[predicted]), 1)
    return cm


def scores(cm):
    """accuracy_score, balanced_accuracy_score (mean recall over the classes that occur), cohen_kappa_score."""
    cm = cm.astype(numpy.float64)
    total = cm.sum()
    oa = numpy.trace(cm) / total
    support = cm.sum(1)
    aa = float(numpy.mean(numpy.diag(cm)[support > 0] / support[support > 0]))
    expected = numpy.outer(cm.sum(1), cm.sum(0)) / total
    off = 1.0 - numpy.eye(len(cm))
    kappa = 1.0 - (off * cm).sum() / (off * expected).sum()
    return float(oa), aa, float(kappa)


def print_output(algorithm_params, average_accuracy, conf_matrix, kappa, overall_accuracy, index, name, base_log_path):
    """reference :139-157"""
    print("OA:%5.5f" % overall_accuracy)
    print("AA:%5.5f" % average_accuracy)
    print("KAPPA:%5.5f" % kappa)
    print("Confusion Matrix:")
    print(conf_matrix)
    file_id = f"{name}_run{index}"
    os.makedirs(base_log_path, exist_ok=True)
    numpy.savetxt(os.path.join(base_log_path, f"confusion_matrix_{file_id}.csv"), conf_matrix, fmt="%d", delimiter=",")
    with open(os.path.join(base_log_path, f"metrics_{file_id}.txt"), "w") as metrics_file:
        print("OA,AA,KAPPA", file=metrics_file)
        print("%.6f,%.6f,%.6f" % (overall_accuracy, average_accuracy, kappa), file=metrics_file)
    with open(os.path.join(base_log_path, f"params_{file_id}.json"), "w") as params_file:
        json.dump(algorithm_params, params_file)


def perform_full_scene_classification(data_path, loader_name, neighborhood, estimator, output_path, pca=None,
                                      profiled=None):
    """reference :83-115: every pixel of the scene, row-major, one (x, y) target each.  pca: the fitted BandPCA of
    --pca_components; the estimator then sees the projected scene.  profiled: the scene --emp_radii computed (after the
    PCA, if any), which is then classified as it is."""
    import torch
    backend = estimator._backend()
    loader = get_loader_from_name(loader_name, data_path)
    if profiled is not None:
        data_set = profiled
    else:
        data_set = loader.load_data(neighborhood, False)
        if pca is not None:
            data_set = pca.transform_scene(data_set)
    scene_shape = data_set.get_scene_shape()
    ys, xs = numpy.meshgrid(numpy.arange(scene_shape[0]), numpy.arange(scene_shape[1]), indexing="ij")
    targets = numpy.stack([xs.reshape(-1), ys.reshape(-1), numpy.zeros(xs.size, dtype=int)], axis=1)
    arrays = SceneArrays()
    arrays.feed(data_set, targets, backend)
    raster = torch.zeros(scene_shape[0] * scene_shape[1], dtype=torch.uint8, device=backend.device)
    estimator.predict_scene(arrays, raster, scene_shape[1])
    scene_as_image = raster.cpu().numpy().reshape(scene_shape[0], scene_shape[1])
    os.makedirs(output_path, exist_ok=True)
    imwrite(os.path.join(output_path, "result_raw.tif"), scene_as_image)
    imwrite(os.path.join(output_path, "result_colorized.tif"),
            create_colored_image(scene_as_image, loader.get_samples_color_list()))
    return scene_as_image


def fit_band_pca(flags, backend=None):
    """--pca_components: one BandPCA per process, fitted on the interior of the loader's scene (it does not depend on
    the split), written as pca_<loader>.json (what was kept and how much of the variance it explains) and
    pca_<loader>.npz (mean_, components_, explained_variance_) next to the result files."""
    from hypelcnn_amd.classic.decomposition import BandPCA
    pca = BandPCA(flags.pca_components, whiten=flags.pca_whiten, backend=backend)
    start_time = time.time()
    pca.fit_scene(get_loader_from_name(flags.loader_name, flags.path).load_data(flags.neighborhood, False))
    print("Completed band PCA: %d of %d bands, %.5f of the variance(%.3f sec)" % (
        pca.n_components_, pca.n_features_in_, pca.explained_variance_ratio_.sum(), time.time() - start_time))
    os.makedirs(flags.base_log_path, exist_ok=True)
    with open(os.path.join(flags.base_log_path, f"pca_{flags.loader_name}.json"), "w") as pca_file:
        json.dump({"n_components": pca.n_components_, "n_samples": pca.n_samples_, "bands": pca.n_features_in_,
                   "whiten": pca.whiten, "explained_variance": pca.explained_variance_.tolist(),
                   "explained_variance_ratio": pca.explained_variance_ratio_.tolist()}, pca_file)
    numpy.savez(os.path.join(flags.base_log_path, f"pca_{flags.loader_name}.npz"), mean_=pca.mean_,
                components_=pca.components_, explained_variance_=pca.explained_variance_)
    return pca


def project_patches(pca, sample_set):
    """[n, p, p, C + lidar] patches -> [n, p, p, k + lidar]: every patch pixel is a row, the LiDAR channels pass through"""
    data = numpy.ascontiguousarray(sample_set.data, dtype=numpy.float32)
    n, p, _, channels = data.shape
    rows = pca.transform(data.reshape(n * p * p, channels), pass_cols=channels - pca.n_features_in_)
    return types.SimpleNamespace(data=rows.reshape(n, p, p, rows.shape[1]), labels=sample_set.labels)


def compute_profile(flags, backend=None, pca=None):
    """--emp_radii: one MorphologicalProfile per process, of the loader's scene behind the PCA (if any); written as
    emp_<loader>.json next to the result files.  -> (the profile, the profiled scene, the loader it came from)"""
    from hypelcnn_amd.classic.morphology import MorphologicalProfile
    profile = MorphologicalProfile(flags.emp_radii, shape=flags.emp_shape, by_reconstruction=not flags.emp_plain,
                                   include_lidar=flags.emp_lidar, backend=backend)
    loader = get_loader_from_name(flags.loader_name, flags.path)
    data_set = loader.load_data(flags.neighborhood, False)
    start_time = time.time()
    if pca is not None:
        data_set = pca.transform_scene(data_set)
    scene = profile.transform_scene(data_set)
    channels = scene.get_casi_band_count()
    levels = 2 * len(profile.radii) + 1
    profile._backend().synchronize()
    seconds = time.time() - start_time
    print("Completed morphological profile: %d bases x %d levels = %d channels, %d sweeps(%.3f sec)" % (
        channels // levels, levels, channels, sum(profile.sweeps_.values()), seconds))
    os.makedirs(flags.base_log_path, exist_ok=True)
    with open(os.path.join(flags.base_log_path, f"emp_{flags.loader_name}.json"), "w") as emp_file:
        json.dump({"radii": list(profile.radii), "shape": profile.shape, "by_reconstruction": profile.by_reconstruction,
                   "include_lidar": profile.include_lidar, "bases": channels // levels, "channels": channels,
                   "sweeps": profile.sweeps_, "seconds": seconds}, emp_file)
    return profile, scene, loader


def cut_profiled_patches(scene, targets, backend):
    """target rows [x, y, class] -> their patches, cut from the profiled scene on the device (what
    InMemoryImporter._get_data_with_labels does on the host for a raw scene)"""
    import torch
    arrays = SceneArrays()
    arrays.feed(scene, targets, backend)
    patches, _ = arrays.gather(torch.arange(len(targets), device=backend.device))
    return types.SimpleNamespace(data=patches.cpu().numpy(), labels=numpy.asarray(targets)[:, 2].astype(numpy.uint8))


def forest_diagnostics_asked(flags):
    return [name for name, on in (("--forest_oob", flags.forest_oob), ("--forest_importances", flags.forest_importances),
                                  ("--forest_permutation_repeats", flags.forest_permutation_repeats > 0)) if on]


def perform_forest_diagnostics(flags, estimator, training, validation, run_index):
    """The forest's own diagnostics, after the reference's three files: forest_diagnostics_<loader>_run<i>.json (the
    out-of-bag score, the rows without a vote, the trees the importances used), band_importance_<loader>_run<i>.csv
    (per band: the impurity importance summed over the window, the permutation mean and standard deviation; nan for
    what was not asked) and feature_importance_<loader>_run<i>.npy ([p, p, channels], with --forest_importances)."""
    p, channels = training.data.shape[1], training.data.shape[3]
    file_id = f"{flags.loader_name}_run{run_index}"
    report = {"estimator": flags.estimator, "oob_score": None, "oob_rows_without_vote": None, "n_used": None,
              "permutation_repeats": flags.forest_permutation_repeats, "permutation_baseline": None}
    per_band = numpy.full((channels, 3), numpy.nan)
    os.makedirs(flags.base_log_path, exist_ok=True)
    if flags.forest_oob:
        report["oob_score"] = estimator.out_of_bag(flatten_data(training.data), training.labels)
        report["oob_rows_without_vote"] = int((estimator.oob_votes_ == 0).sum())
        print("OOB:%5.5f" % report["oob_score"])
    if flags.forest_importances:
        importances = estimator.feature_importances().reshape(p, p, channels)
        report["n_used"] = estimator.importances_n_used_
        per_band[:, 0] = importances.sum((0, 1))
        numpy.save(os.path.join(flags.base_log_path, f"feature_importance_{file_id}.npy"), importances)
    if flags.forest_permutation_repeats > 0:
        result = estimator.permutation_importance(flatten_data(validation.data), validation.labels,
                                                  n_repeats=flags.forest_permutation_repeats, group_mod=channels,
                                                  seed=flags.forest_seed + run_index)
        report["permutation_baseline"] = result["baseline"]
        per_band[:, 1], per_band[:, 2] = result["importances_mean"], result["importances_std"]
    if flags.forest_importances or flags.forest_permutation_repeats > 0:
        with open(os.path.join(flags.base_log_path, f"band_importance_{file_id}.csv"), "w") as band_file:
            print("band,impurity_importance,permutation_mean,permutation_std", file=band_file)
            for band, row in enumerate(per_band):
                print("%d,%.17g,%.17g,%.17g" % (band, *row), file=band_file)
    with open(os.path.join(flags.base_log_path, f"forest_diagnostics_{file_id}.json"), "w") as report_file:
        json.dump(report, report_file)
    return report


def parse_decades(text, flag):
    """'lo:hi:n' -> numpy.logspace(lo, hi, n), the form of the reference's two ranges (:127-128)"""
    try:
        lo, hi, n = text.split(":")
        lo, hi, n = float(lo), float(hi), int(n)
    except ValueError:
        raise ValueError(f"{flag} {text!r}: decades as lo:hi:n, e.g. -2:10:13") from None
    if n < 1:
        raise ValueError(f"{flag} {text!r}: n >= 1")
    return numpy.logspace(lo, hi, n)


last_grid_search = None  # the GridSearchSVC of the most recent --svc_grid run (also estimator.grid_search_)


def perform_grid_search(flags, data, labels, run_index, backend=None):
    """reference :126-136 on the device; the reference's print line, and the result as a JSON file next to the metrics."""
    from hypelcnn_amd.classic.model_selection import GridSearchSVC, StratifiedShuffleSplit
    global last_grid_search
    param_grid = {"C": parse_decades(flags.svc_grid_c, "--svc_grid_c"),
                  "gamma": parse_decades(flags.svc_grid_gamma, "--svc_grid_gamma")}
    cv = StratifiedShuffleSplit(n_splits=2, test_size=0.1, random_state=42)
    start_time = time.time()
    grid = GridSearchSVC(param_grid, cv, tol=flags.svc_tol, refit=flags.svc_grid_refit, backend=backend).fit(data, labels)
    print("Completed grid search(%.3f sec)" % (time.time() - start_time))
    print("The best parameters are %s with a score of %0.2f" % (grid.best_params_, grid.best_score_))
    res = grid.cv_results_
    nan_to_none = lambda a: [None if numpy.isnan(v) else float(v) for v in a]  # noqa: E731 -- JSON has no NaN
    out = {"params": res["params"], "mean_test_score": nan_to_none(res["mean_test_score"]),
           "rank_test_score": res["rank_test_score"].tolist(), "best_index": grid.best_index_,
           "best_params": grid.best_params_, "best_score": grid.best_score_, "n_splits": grid.n_splits_,
           "unconverged_cells": [i for i, v in enumerate(res["mean_test_score"]) if numpy.isnan(v)]}
    for split in range(grid.n_splits_):
        out[f"split{split}_test_score"] = nan_to_none(res[f"split{split}_test_score"])
    os.makedirs(flags.base_log_path, exist_ok=True)
    with open(os.path.join(flags.base_log_path, f"svc_grid_{flags.loader_name}_run{run_index}.json"), "w") as grid_file:
        json.dump(out, grid_file)
    last_grid_search = grid
    return grid


def build_parser():
    parser = argparse.ArgumentParser()
    add_parse_cmds_for_loaders(parser)
    add_parse_cmds_for_loggers(parser)
    add_parse_cmds_for_app(parser)
    add_parse_cmds_for_trainers(parser)
    return parser


def join_decade_values(argv):
    """`--svc_grid_c -2:10:13`: argparse takes a value that starts with '-' and is not a number for an option and leaves
    the flag empty, so the two decade flags are handed over in their `--flag=value` form."""
    argv = list(sys.argv[1:] if argv is None else argv)
    out = []
    while argv:
        token = argv.pop(0)
        if token in ("--svc_grid_c", "--svc_grid_gamma") and argv:
            token += "=" + argv.pop(0)
        out.append(token)
    return out


def main(argv=None, backend=None):
    flags, _ = build_parser().parse_known_args(join_decade_values(argv))
    if flags.hyperparamopt:
        raise NotImplementedError(
            "--hyperparamopt (reference classic_ml_trainer.py:126-136) is not built: its contract is scikit-learn's own "
            "GridSearchCV object; the same search, with the same grid and splits, runs on the device under --svc_grid "
            "(--svc_grid_c / --svc_grid_gamma / --svc_grid_refit)")
    if flags.svc_grid and flags.estimator in ("forest", "extra_trees"):
        raise ValueError(f"--svc_grid searches the SVC's C x gamma: not with --estimator {flags.estimator}")
    if forest_diagnostics_asked(flags) and flags.estimator not in ("forest", "extra_trees"):
        raise ValueError(f"{', '.join(forest_diagnostics_asked(flags))}: diagnostics of a forest (--estimator forest or "
                         f"extra_trees), not of --estimator {flags.estimator}")
    results = []
    pca = fit_band_pca(flags, backend) if flags.pca_components else None
    profile, profiled, profiled_loader = compute_profile(flags, backend, pca) if flags.emp_radii else (None, None, None)
    for run_index in range(flags.split_count):
        print("Starting episode#%d" % run_index)
        if profile is not None:
            # a profile is no per-pixel function: the patches are cut from the profiled scene, at the targets
            # InMemoryImporter.read_data_set would have cut from the raw one
            sample_set = profiled_loader.load_samples(0.1, 0)
            training = cut_profiled_patches(profiled, sample_set.training_targets, profile._backend())
            validation = cut_profiled_patches(profiled, sample_set.validation_targets, profile._backend())
        else:
            training, _, validation, _, _, _, _ = InMemoryImporter().read_data_set(
                loader_name=flags.loader_name, path=flags.path, test_data_ratio=0, train_data_ratio=0.1,
                neighborhood=flags.neighborhood, normalize=False)
            if pca is not None:
                training, validation = project_patches(pca, training), project_patches(pca, validation)
        start_time = time.time()
        estimator = create_estimator(flags, backend, run_index)
        estimator.fit(flatten_data(training.data), training.labels)
        print("Completed training(%.3f sec)" % (time.time() - start_time))
        predicted = estimator.predict(flatten_data(validation.data))
        conf_matrix = confusion_matrix(validation.labels, predicted)
        overall_accuracy, average_accuracy, kappa = scores(conf_matrix)
        print_output(estimator.get_params(), average_accuracy, conf_matrix, kappa, overall_accuracy, run_index,
                     flags.loader_name, flags.base_log_path)
        if forest_diagnostics_asked(flags):
            estimator.diagnostics_ = perform_forest_diagnostics(flags, estimator, training, validation, run_index)
        if flags.svc_grid:
            grid = perform_grid_search(flags, flatten_data(training.data), training.labels, run_index, backend)
            if flags.svc_grid_refit:
                estimator = grid.best_estimator_
            estimator.grid_search_ = grid
        scene = None
        if flags.fullscene:
            scene = perform_full_scene_classification(flags.path, flags.loader_name, flags.neighborhood, estimator,
                                                      flags.output_path, pca, profiled)
        results.append((estimator, predicted, conf_matrix, (overall_accuracy, average_accuracy, kappa), scene))
    return results


if __name__ == "__main__":
    main()
