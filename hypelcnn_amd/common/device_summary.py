"""tf.summary.histogram of the model variables, computed where they live (include/hypel.h hypel_tensor_summary_f32).

The variables of a session are segments of two flat device buffers (Session.params: trainable, Session.state: batch-norm
moving statistics); one launch per buffer summarises all of its variables.  Only the per-variable results come back:
5 doubles, the non-finite count and the bucket counts (1551 int64 = 12 KiB per variable; ~1 MiB for a hundred
variables every summary step, against the ~1 GB of DUALCNN's parameters the host path copies)."""
import numpy
import torch

from hypelcnn_amd.backend import SUMMARY_SLICE, Ref
from hypelcnn_amd.common.tb_events import default_bucket_limits


def summary_slices(sizes):
    """ws_slices of hypel_tensor_summary_f32 for segments of these sizes"""
    return int(sum((int(s) + SUMMARY_SLICE - 1) // SUMMARY_SLICE for s in sizes if s > 0))


class TensorSummary:
    """The launch over one base buffer: `segments` = [(element offset, size)]."""

    def __init__(self, backend, base, segments, limits_dev, n_limits):
        self.be, self.base, self.n, self.n_limits = backend, base, len(segments), int(n_limits)
        table = numpy.asarray(segments, numpy.int64).reshape(self.n, 2)
        assert (table >= 0).all() and int((table[:, 0] + table[:, 1]).max()) <= base.numel()
        self.slices = summary_slices(table[:, 1])
        self.table = backend.upload(table)
        self.limits = limits_dev
        self.stats = backend.zeros(5 * self.n, torch.float64)
        self.nonfinite = backend.zeros(self.n, torch.int64)
        self.buckets = backend.zeros(self.n * self.n_limits, torch.int64)
        self.ws = backend.zeros(self.n + 1 + 6 * self.slices, torch.float64)  # HYPEL_SUMMARY_WS_DOUBLES

    def launch(self):
        self.be.call("tensor_summary_f32", Ref(self.base), Ref(self.table), self.n, Ref(self.limits), self.n_limits,
                     Ref(self.stats), Ref(self.nonfinite), Ref(self.buckets), Ref(self.ws), self.slices)

    def results(self):
        """-> stats [n, 5] float64 (min, max, num, sum, sum_squares), nonfinite [n] int64, buckets [n, n_limits]"""
        nonfinite = self.nonfinite.cpu().numpy()
        if (nonfinite < 0).any():
            raise RuntimeError("hypel_tensor_summary_f32 refused its segment table (slice count mismatch)")
        return (self.stats.cpu().numpy().reshape(self.n, 5), nonfinite,
                self.buckets.cpu().numpy().reshape(self.n, self.n_limits))


class VariableSummarizer:
    """Histograms of every variable of a Session (what a checkpoint saves under nn_core/*: the trainable variables and
    the batch-norm moving statistics; no optimiser slots)."""

    def __init__(self, sess):
        self.limits = default_bucket_limits()
        be = sess.backend
        limits_dev = be.upload(self.limits)
        self.parts = []
        for base, variables in ((sess.params, sess.trainable), (sess.state, sess.stateful)):
            if variables:
                self.parts.append(([v.name for v in variables],
                                   TensorSummary(be, base, [(v.offset, v.size) for v in variables], limits_dev,
                                                 self.limits.size)))

    def launch(self):
        for _, part in self.parts:
            part.launch()

    def run(self):
        """{variable name: {"min", "max", "num", "sum", "sum_squares", "nonfinite", "buckets" (int64 [n_limits])}}"""
        self.launch()
        out = {}
        for names, part in self.parts:
            stats, nonfinite, buckets = part.results()
            for i, name in enumerate(names):
                out[name] = {"min": float(stats[i, 0]), "max": float(stats[i, 1]), "num": float(stats[i, 2]),
                             "sum": float(stats[i, 3]), "sum_squares": float(stats[i, 4]),
                             "nonfinite": int(nonfinite[i]), "buckets": buckets[i]}
        return out
