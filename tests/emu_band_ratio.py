"""TEST INFRASTRUCTURE: numpy twins of the band-ratio entry points (include/hypel.h, hypel_band_ratio_f32 and
hypel_column_rank_select_f32), attached to tests/emu_backend.EmuBackend on import.  Written from the header: buffers have
the device's dtypes and layouts, the arithmetic is NumPy's own.
Every launch is appended to the backend's `launch_log`."""
import numpy as np

from hypelcnn_amd.backend import COLUMN_RANK_MAX_RANKS, COLUMN_RANK_WS_WORDS
from tests.emu_backend import EmuBackend
from tests.emu_scene import _typed


def _matrix(ref, ld, n, bands):
    flat = _typed(ref, np.float32)
    assert ld >= bands and (n - 1) * ld + bands <= flat.size, "the strided matrix reaches past its buffer"
    return np.lib.stride_tricks.as_strided(flat, shape=(n, bands), strides=(ld * 4, 4))


def _k_band_ratio_f32(self, num, ld_num, den, ld_den, n, bands, scale, ratio, ld_ratio, row_ok, kept):
    assert 1 <= n < 2 ** 31 and bands >= 1
    a, d = _matrix(num, ld_num, n, bands), _matrix(den, ld_den, n, bands)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        r = a / d
        if scale is not None:
            r = r * _typed(scale, np.float32, bands)
    assert r.dtype == np.float32
    _matrix(ratio, ld_ratio, n, bands)[...] = r
    ok = np.isfinite(r).all(axis=1)
    _typed(row_ok, np.uint8, n)[:] = ok
    _typed(kept, np.int64, 1)[0] = int(ok.sum())
    self.launch_log.append("band_ratio_f32")


def _k_column_rank_select_f32(self, x, ld, n, bands, row_ok, kept, ranks, n_ranks, out, ws):
    assert 1 <= n < 2 ** 31 and bands >= 1 and 1 <= n_ranks <= COLUMN_RANK_MAX_RANKS
    assert _typed(ws, np.uint32).size >= bands * COLUMN_RANK_WS_WORDS
    rows = _matrix(x, ld, n, bands)
    if row_ok is not None:
        rows = rows[_typed(row_ok, np.uint8, n) != 0]
    assert rows.shape[0] == kept >= 1 and np.isfinite(rows).all()
    want = _typed(ranks, np.int64, n_ranks)
    assert ((0 <= want) & (want < kept)).all()
    _typed(out, np.float32, n_ranks * bands).reshape(n_ranks, bands)[...] = np.sort(rows, axis=0)[want]
    self.launch_log.append("column_rank_select_f32")


for _name, _fn in list(globals().items()):
    if _name.startswith("_k_band_ratio") or _name.startswith("_k_column_rank"):
        setattr(EmuBackend, _name[1:], _fn)
