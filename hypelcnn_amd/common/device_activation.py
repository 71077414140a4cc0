"""Histograms of a tower's tapped activations, taken where the forward pass leaves them (include/hypel.h
hypel_view_range_f32 / hypel_view_histogram_f32).

A tap lies in a pixel-major plan buffer [npix][nb][ld] (TowerPlan.storage_of: ch_off, c, ld, optionally a pixmap), so it
is one strided view of npix * nb rows -- or one view per run of consecutive pixels of its pixmap -- and both launches
accumulate: a tap is folded over as many batches and views as there are.  Two passes, because the bins lie between the
tap's global extremes: fold_range() after every forward, set_edges() once (one small copy to the host), then
fold_histogram() after every forward.  Only the per-tap results ever leave the device."""
import numpy
import torch

from hypelcnn_amd.backend import ACT_MAX_BINS, Ref

FLT_MAX = float(numpy.finfo(numpy.float32).max)


def tap_size(sym):
    """elements of one sample of a tapped tensor (the reference's calculate_tensor_size: the batch dimension is None)"""
    return int(sym.features) if hasattr(sym, "sources") else int(sym.npix * sym.c)


def tap_bins(taps, base_bins=480):
    """{name: bins} -- the reference's int(base_bins / size_0 * size_i), at least 1 (the reference asks numpy for 0 bins
    there); a tap that needs more than HYPEL_ACT_MAX_BINS is refused by name"""
    first = tap_size(taps[0][0])
    bins = {}
    for sym, name in taps:
        n = max(1, int(base_bins / first * tap_size(sym)))
        if n > ACT_MAX_BINS:
            raise ValueError(f"tap {name!r} needs {n} bins, more than the {ACT_MAX_BINS} a histogram launch holds "
                             f"(HYPEL_ACT_MAX_BINS): lower --base_bins")
        bins[name] = n
    return bins


def storage_views(st, nb):
    """[(element offset, rows)] of a Storage: the views of `c` columns and leading dimension `ld` that cover it"""
    if st.pixmap is None:
        return [(st.ch_off, st.npix * nb)]
    runs, pm = [], list(st.pixmap)
    start = 0
    for i in range(1, len(pm) + 1):
        if i == len(pm) or pm[i] != pm[i - 1] + 1:
            runs.append((pm[start] * nb * st.ld + st.ch_off, (i - start) * nb))
            start = i
    return runs


class ActivationTaps:
    """taps: [(sym, name)] of ONE tower (ModelOutputTensors.histogram_tensors); bins: {name: bins} or one int."""

    def __init__(self, sess, taps, bins=480):
        self.be = sess.backend
        self.taps = [(sym, name) for sym, name in taps]
        self.names = [name for _, name in self.taps]
        self.bins = {n: int(bins[n] if isinstance(bins, dict) else bins) for n in self.names}
        for name, n in self.bins.items():
            if not 1 <= n <= ACT_MAX_BINS:
                raise ValueError(f"tap {name!r}: {n} bins, outside 1 .. {ACT_MAX_BINS} (HYPEL_ACT_MAX_BINS)")
        k = len(self.taps)
        self.range = self.be.upload(numpy.tile(numpy.asarray([FLT_MAX, -FLT_MAX], numpy.float32), k))
        self.count = self.be.zeros(2 * k, torch.int64)
        self.outside = self.be.zeros(k, torch.int64)
        self.counts = [self.be.zeros(self.bins[n], torch.int64) for n in self.names]
        self.edges_dev = None
        self.edges = None

    def _views(self, ct, sym):
        """(buffer, element offset, rows, ld, cols) of every view of a tap in a compiled tower"""
        out = []
        for s in (sym.sources if hasattr(sym, "sources") else [sym]):
            st = ct.plan.storage_of(s)
            for off, rows in storage_views(st, ct.plan.nb):
                out.append((ct.plan.buffers[st.buf], off, rows, st.ld, st.c))
        return out

    def fold_range(self, ct):
        """after ct.forward(): fold every tap's extremes and element counts"""
        for i, (sym, _) in enumerate(self.taps):
            for buf, off, rows, ld, cols in self._views(ct, sym):
                self.be.call("view_range_f32", Ref(buf, off), rows, ld, cols, Ref(self.range, 2 * i),
                             Ref(self.count, 2 * i))

    def set_edges(self):
        """bins + 1 uniform float64 edges between every tap's folded extremes: numpy.histogram's, with its (lo - 0.5,
        hi + 0.5) for a tap of one value"""
        ranges = self.range.cpu().numpy().reshape(-1, 2)
        self.edges, self.edges_dev = {}, {}
        for (lo, hi), name in zip(ranges, self.names):
            if lo > hi:
                raise ValueError(f"tap {name!r} has no finite element to take a range from")
            lo, hi = float(lo) + 0.0, float(hi) + 0.0
            if lo == hi:
                lo, hi = lo - 0.5, hi + 0.5
            self.edges[name] = numpy.linspace(lo, hi, self.bins[name] + 1)
            self.edges_dev[name] = self.be.upload(self.edges[name])
        return self.edges

    def fold_histogram(self, ct):
        """after ct.forward(), once set_edges() has run: add every tap's elements to its bins"""
        if self.edges_dev is None:
            raise RuntimeError("ActivationTaps.fold_histogram before set_edges")
        for i, (sym, name) in enumerate(self.taps):
            for buf, off, rows, ld, cols in self._views(ct, sym):
                self.be.call("view_histogram_f32", Ref(buf, off), rows, ld, cols, Ref(self.edges_dev[name]),
                             self.bins[name], Ref(self.counts[i]), Ref(self.outside, i))

    def results(self):
        """{name: {"lo", "hi", "edges" (float64 [bins + 1]), "counts" (int64 [bins]), "finite", "nonfinite",
        "outside"}}"""
        ranges = self.range.cpu().numpy().reshape(-1, 2)
        count = self.count.cpu().numpy().reshape(-1, 2)
        outside = self.outside.cpu().numpy()
        out = {}
        for i, name in enumerate(self.names):
            out[name] = {"lo": float(ranges[i, 0]) + 0.0, "hi": float(ranges[i, 1]) + 0.0,
                         "edges": None if self.edges is None else self.edges[name],
                         "counts": self.counts[i].cpu().numpy().copy(), "finite": int(count[i, 0]),
                         "nonfinite": int(count[i, 1]), "outside": int(outside[i])}
        return out
