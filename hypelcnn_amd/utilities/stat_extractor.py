"""OA / AA / kappa tables from confusion matrices (reference utilities/stat_extractor.py), the last step of the chain
event file -> read_summary_file -> CSV -> stat_extractor:

    python -m hypelcnn_amd.utilities.stat_extractor <directory of *.csv confusion matrices>

The reference's functions under their names, with its behaviour kept: rows are the true classes, a class without
samples gives a NaN class accuracy, and extract_statistics_info files run k's metrics at index k - 1 (the first run
lands in the last slot)."""
import glob
import os
import sys
from collections import namedtuple

import numpy

MetricsHolder = namedtuple("MetricsHolder", ["aa_array", "kappa_array", "oa_array", "sample_count"])


def histogram(confusion_matrix, index):
    """Totals of the rows (index 0) or of the columns (index 1)."""
    confusion_matrix = numpy.asarray(confusion_matrix)
    return confusion_matrix.sum(axis=1 - index).astype(int)[:confusion_matrix.shape[index]]


def calc_kappa(conf_mat):
    """Cohen's kappa with 0 / 1 disagreement weights: 1 - observed disagreement / disagreement expected by chance."""
    conf_mat = numpy.asarray(conf_mat)
    rows = histogram(conf_mat, 0).astype(float)
    cols = histogram(conf_mat, 1).astype(float)
    total = float(rows.sum())
    off_diagonal = ~numpy.eye(len(conf_mat), dtype=bool)
    numerator = (conf_mat / total)[off_diagonal].sum()
    denominator = (numpy.outer(rows, cols) / total / total)[off_diagonal].sum()
    return 1.0 - numerator / denominator


def calc_mean_quadratic_weighted_kappa(kappas, weights=None):
    """Mean of kappas in Fisher's z space (kappas capped to [-0.999, 0.999]; weights, normalised to mean 1, apply in z)."""
    kappas = numpy.clip(numpy.array(kappas, dtype=float), -.999, .999)
    weights = numpy.ones(kappas.shape) if weights is None else weights / numpy.mean(weights)
    z = numpy.mean(0.5 * numpy.log((1 + kappas) / (1 - kappas)) * weights)
    return (numpy.exp(2 * z) - 1) / (numpy.exp(2 * z) + 1)


def extract_accuracy_metrics(confusion_matrix):
    """-> overall accuracy, per-class accuracy (diagonal / row total), kappa, samples per class (row totals)"""
    confusion_matrix = numpy.asarray(confusion_matrix)
    overall_accuracy = numpy.trace(confusion_matrix) / numpy.sum(confusion_matrix)
    class_based_samples = confusion_matrix.sum(axis=1).astype(int)
    with numpy.errstate(divide="ignore", invalid="ignore"):
        class_accuracy = numpy.diagonal(confusion_matrix) / class_based_samples.astype(float)
    return overall_accuracy, class_accuracy, calc_kappa(confusion_matrix), class_based_samples


def extract_statistics_info(confusion_matrix_list):
    oa_array = aa_array = kappa_array = sample_count = None
    file_count = len(confusion_matrix_list)
    for index, confusion_matrix in enumerate(confusion_matrix_list):
        oa, aa, kappa, class_based_samples = extract_accuracy_metrics(confusion_matrix)
        if oa_array is None:
            oa_array = numpy.zeros(file_count, dtype=float)
            aa_array = numpy.zeros([file_count, aa.shape[0]], dtype=float)
            kappa_array = numpy.zeros(file_count, dtype=float)
            sample_count = class_based_samples
        oa_array[index - 1] = oa  # the reference's placement: run 0 in the last slot
        aa_array[index - 1, :] = aa
        kappa_array[index - 1] = kappa
    return MetricsHolder(aa_array=aa_array, kappa_array=kappa_array, oa_array=oa_array, sample_count=sample_count)


def get_conf_list_from_directory(directory):
    return [numpy.loadtxt(filename, dtype=int, delimiter=",", ndmin=2)
            for filename in glob.glob(os.path.join(directory, "*.csv"))]


def calculate_mean_std_metrics(oa_array, aa_array, kappa_array):
    run_aa = numpy.mean(aa_array, axis=1)
    return numpy.mean(oa_array), numpy.std(oa_array), numpy.mean(run_aa), numpy.std(run_aa), \
        numpy.mean(kappa_array), numpy.std(kappa_array)


def print_statistics_info(metrics_holder):
    if metrics_holder.oa_array is None:
        print("#No confusion matrices")
        return
    for oa, aa, kappa in zip(metrics_holder.oa_array, metrics_holder.aa_array, metrics_holder.kappa_array):
        print("OA: %.4f AA: %.4f Kappa: %.4f" % (oa, numpy.mean(aa), kappa))
    print("#Metrics statistics:")
    mean_oa, std_oa, mean_aa, std_aa, mean_kappa, std_kappa = calculate_mean_std_metrics(
        metrics_holder.oa_array, metrics_holder.aa_array, metrics_holder.kappa_array)
    print("OA:    %.4f +- %.4f" % (mean_oa, std_oa))
    print("AA:    %.4f +- %.4f" % (mean_aa, std_aa))
    print("Kappa: %.4f +- %.4f" % (mean_kappa, std_kappa))
    print("#Class based accuracy")
    for aa_mean, aa_std, a_sample_count in zip(numpy.mean(metrics_holder.aa_array, axis=0),
                                               numpy.std(metrics_holder.aa_array, axis=0), metrics_holder.sample_count):
        print("%.4f +- %.4f %d" % (aa_mean, aa_std, a_sample_count))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    print_statistics_info(extract_statistics_info(get_conf_list_from_directory(argv[0])))


if __name__ == "__main__":
    main()
