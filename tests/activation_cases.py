"""TEST INFRASTRUCTURE: inputs of the activation range / histogram tests (include/hypel.h: hypel_view_range_f32,
hypel_view_histogram_f32) and their float64 NumPy reference, shared by the host tests (EmuBackend with the twin of
tests/emu_activation.py) and the GPU tests (HipBackend).

A case is a rows x cols view at an element offset of a buffer filled with SENTINEL (a finite value outside every edge
table here: one element read from a gap shows in `outside`, in `finite` and in the maximum), an edge table, and values
that hold every edge's float32 neighbourhood (the float32 at or below it, the one above, and the next one), +-0, NaN,
+-Inf and finite values outside the table; the rest is drawn from a palette of a few thousand values in range, so that
the references stay quick on the large views.  The reference is numpy.histogram on the float64 values: with `bins` and
`range` for a uniform table -- the call the tool has to meet -- and with the edge array for the other one."""
import functools
from collections import namedtuple

import numpy as np
import torch

from hypelcnn_amd.backend import ACT_MAX_BINS, Ref

FLT_MAX = np.finfo(np.float32).max
SENTINEL = np.float32(12345.0)
LO, HI = -1.5, 2.75
SPECIALS = np.asarray([0.0, -0.0, np.nan, np.inf, -np.inf, np.nan, -7.0, 1e30, -FLT_MAX, 2.7500002, -1.5000001],
                      np.float32)  # five finite values outside [LO, HI], four non-finite ones

Case = namedtuple("Case", "name rows cols ld off edges uniform buffer values counts outside finite nonfinite lo hi")

# name: rows, cols, ld, element offset, bins (an int: uniform between LO and HI; "table": the non-uniform one)
SPECS = {
    "1x1": (1, 1, 1, 0, 1),
    "1x1_strided": (1, 1, 5, 3, 2),
    "1x63": (1, 63, 63, 0, 3),
    "1x63_strided": (1, 63, 70, 1, 480),
    "3x64": (3, 64, 64, 0, 481),
    "3x64_strided": (3, 64, 67, 5, 2),
    "5x65_odd_offset": (5, 65, 65, 1, 480),
    "5x65_strided": (5, 65, 66, 7, 1),
    "5x65_table": (5, 65, 65, 3, "table"),
    "4097x3": (4097, 3, 3, 0, ACT_MAX_BINS),
    "4097x3_strided": (4097, 3, 4, 1, 481),
    "3x5000_strided": (3, 5000, 5003, 1, 480),  # rows longer than one wavefront's span
    "70000x33": (70000, 33, 33, 0, ACT_MAX_BINS),
    "70000x33_odd_offset": (70000, 33, 33, 1, 480),
    "70000x33_strided": (70000, 33, 40, 3, 481),
    "70000x33_strided_3": (70000, 33, 35, 1, 3),
    "70000x33_table": (70000, 33, 36, 5, "table"),
}
NAMES = sorted(SPECS)


def uniform_edges(bins, lo=LO, hi=HI):
    return np.linspace(float(lo), float(hi), bins + 1)


def table_edges():
    """37 bins whose widths span four decades, strictly ascending between LO and HI"""
    rng = np.random.default_rng(5)
    widths = 10.0 ** rng.uniform(-4, 0, 37)
    edges = LO + (HI - LO) * np.concatenate([[0.0], np.cumsum(widths) / widths.sum()])
    edges[-1] = HI
    assert (np.diff(edges) > 0).all()
    return edges


def edge_neighbours(edges):
    """for every edge: the float32 at or below it, the next float32 and the one after that"""
    with np.errstate(over="ignore"):
        near = edges.astype(np.float32)
    below = np.where(near.astype(np.float64) <= edges, near, np.nextafter(near, np.float32(-np.inf)))
    above = np.nextafter(below, np.float32(np.inf))
    return np.concatenate([below, above, np.nextafter(above, np.float32(np.inf))]).astype(np.float32)


def reference(values, edges, uniform):
    """-> counts, outside, finite, nonfinite, lo, hi of float32 values: numpy.histogram on the float64 values"""
    v = np.asarray(values, np.float32).reshape(-1)
    d = v[np.isfinite(v)].astype(np.float64)
    inside = d[(d >= edges[0]) & (d <= edges[-1])]
    if uniform:
        counts, made = np.histogram(inside, bins=len(edges) - 1, range=(float(edges[0]), float(edges[-1])))
        assert np.array_equal(made, edges)
    else:
        counts, _ = np.histogram(inside, bins=edges)
    lo, hi = (float(d.min()), float(d.max())) if d.size else (float(FLT_MAX), -float(FLT_MAX))
    return counts.astype(np.int64), int(d.size - inside.size), int(d.size), int(v.size - d.size), lo, hi


def place(values, rows, cols, ld, off):
    """the rows x cols values as a view at `off` of a SENTINEL-filled buffer"""
    buf = np.full(off + rows * ld + 9, SENTINEL, np.float32)
    view = np.lib.stride_tricks.as_strided(buf[off:], (rows, cols), (4 * ld, 4))
    view[...] = np.asarray(values, np.float32).reshape(rows, cols)
    return buf


@functools.lru_cache(maxsize=None)
def case(name):
    rows, cols, ld, off, bins = SPECS[name]
    uniform = bins != "table"
    edges = uniform_edges(bins) if uniform else table_edges()
    rng = np.random.default_rng(sum(name.encode()))
    n = rows * cols
    must = np.concatenate([SPECIALS, edge_neighbours(edges)])
    palette = np.concatenate([must, rng.uniform(LO, HI, 2000).astype(np.float32)])
    values = np.concatenate([must, palette[rng.integers(0, palette.size, max(n - must.size, 0))]])[:n]
    values = values[rng.permutation(n)]
    counts, outside, finite, nonfinite, lo, hi = reference(values, edges, uniform)
    return Case(name, rows, cols, ld, off, edges, uniform, place(values, rows, cols, ld, off), values, counts, outside,
                finite, nonfinite, lo, hi)


def fresh_outputs(be, n_bins):
    """range (+FLT_MAX, -FLT_MAX), count [2], counts [n_bins], outside [1] as the caller of the launches starts them"""
    return {"range": be.upload(np.asarray([FLT_MAX, -FLT_MAX], np.float32)), "count": be.zeros(2, torch.int64),
            "counts": be.zeros(n_bins, torch.int64), "outside": be.zeros(1, torch.int64)}


def fold(be, out, buffer_dev, off, rows, ld, cols, edges_dev, n_bins):
    """both launches on one view, into `out`"""
    be.call("view_range_f32", Ref(buffer_dev, off), rows, ld, cols, Ref(out["range"]), Ref(out["count"]))
    be.call("view_histogram_f32", Ref(buffer_dev, off), rows, ld, cols, Ref(edges_dev), n_bins, Ref(out["counts"]),
            Ref(out["outside"]))


def fetch(be, out):
    be.synchronize()
    r, c = out["range"].cpu().numpy(), out["count"].cpu().numpy()
    return {"lo": float(r[0]), "hi": float(r[1]), "finite": int(c[0]), "nonfinite": int(c[1]),
            "counts": out["counts"].cpu().numpy(), "outside": int(out["outside"].cpu().numpy()[0])}


def run_case(be, c):
    out = fresh_outputs(be, len(c.edges) - 1)
    fold(be, out, be.upload(c.buffer), c.off, c.rows, c.ld, c.cols, be.upload(c.edges), len(c.edges) - 1)
    return fetch(be, out)


def check(got, counts, outside, finite, nonfinite, lo, hi, where=""):
    """every figure is compared exactly (the extremes by value: -0.0 equals 0.0)"""
    diff = np.flatnonzero(got["counts"] != counts)
    assert diff.size == 0, (where, diff[:8], got["counts"][diff[:8]], counts[diff[:8]])
    assert (got["outside"], got["finite"], got["nonfinite"]) == (outside, finite, nonfinite), where
    assert got["lo"] == lo and got["hi"] == hi, (where, got["lo"], got["hi"], lo, hi)


def check_case(got, c):
    check(got, c.counts, c.outside, c.finite, c.nonfinite, c.lo, c.hi, c.name)
    assert int(got["counts"].sum()) + got["outside"] == got["finite"], c.name


# ---- contention: 2^22 elements of one value, and of two alternating values --------------------------------------
N_CONTENTION = 2 ** 22


@functools.lru_cache(maxsize=None)
def contention(kind):
    """-> values, edges (480 uniform bins over the values' own range, numpy's (v - 0.5, v + 0.5) for a single value)"""
    if kind == "one":
        values, lo, hi = np.full(N_CONTENTION, 0.0371, np.float32), np.float32(0.0371) - 0.5, np.float32(0.0371) + 0.5
    else:
        values = np.tile(np.asarray([0.0371, -1.25], np.float32), N_CONTENTION // 2)
        lo, hi = -1.25, np.float32(0.0371)
    return values, uniform_edges(480, float(lo), float(hi))
