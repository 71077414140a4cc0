"""TEST INFRASTRUCTURE: numpy twin of the activation entry points (include/hypel.h: hypel_view_range_f32,
hypel_view_histogram_f32), attached to tests/emu_backend.EmuBackend on import.  Written from the header, by other means
than the reference of tests/activation_cases.py (numpy.histogram): the bin of a value in range is the NUMBER of interior
edges at or below it, counted edge by edge on the float64 values (once per distinct value), not a search."""
import numpy as np

from hypelcnn_amd.backend import ACT_MAX_BINS
from tests.emu_backend import EmuBackend
from tests.emu_scene import _typed


def _view(src, rows, ld, cols):
    assert rows >= 0 and cols >= 1 and ld >= cols and rows * cols < 2 ** 37
    flat = _typed(src, np.float32)
    if rows == 0:
        return np.zeros(0, np.float32)
    assert (rows - 1) * ld + cols <= flat.size, "the view reaches past its buffer"
    return np.lib.stride_tricks.as_strided(flat, (rows, cols), (4 * ld, 4)).reshape(-1)


def _k_view_range_f32(self, src, rows, ld, cols, range, count):  # noqa: A002 -- the header's parameter names
    v = _view(src, rows, ld, cols)
    fin = np.isfinite(v)
    r, c = _typed(range, np.float32, 2), _typed(count, np.int64, 2)
    if fin.any():
        r[0], r[1] = min(r[0], v[fin].min()), max(r[1], v[fin].max())
    c[0] += int(fin.sum())
    c[1] += int(v.size - fin.sum())


def _k_view_histogram_f32(self, src, rows, ld, cols, edges, n_bins, counts, outside):
    assert 1 <= n_bins <= ACT_MAX_BINS
    e = _typed(edges, np.float64, n_bins + 1)
    assert (np.diff(e) > 0).all(), "the edges are strictly ascending"
    v = _view(src, rows, ld, cols)
    d = v[np.isfinite(v)].astype(np.float64)
    inside = (d >= e[0]) & (d <= e[n_bins])
    distinct, times = np.unique(d[inside], return_counts=True)
    cnt = _typed(counts, np.int64, n_bins)
    interior = e[1:n_bins]
    for start in range(0, distinct.size, 2048):
        part = distinct[start:start + 2048]
        bins = (interior[None, :] <= part[:, None]).sum(axis=1)
        np.add.at(cnt, bins, times[start:start + 2048])
    _typed(outside, np.int64, 1)[0] += int(d.size - inside.sum())


for _name, _fn in list(globals().items()):
    if _name.startswith("_k_"):
        setattr(EmuBackend, _name[1:], _fn)
