"""CPU: the band-ratio entry points are declared in include/hypel.h, exported by the library (their binding:
tests/test_abi.py, which checks every prototype of the header), publish their workspace size in both places, and refuse
bad arguments by name before anything is launched.  The ABI version is still 8: new symbols only."""
import ctypes
import re

from tests.test_abi import HEADER, _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_band_ratio_f32", "hypel_column_rank_select_f32")


def test_version_8_and_new_symbols(lib):  # noqa: F811
    from hypelcnn_amd import backend
    src = open(HEADER).read()
    header = int(re.search(r"#define\s+HYPEL_ABI_VERSION\s+(\d+)", src).group(1))
    assert header == backend.ABI_VERSION == lib.hypel_version() == 8
    decl = _declared()
    for name in NEW:
        assert name in decl and hasattr(lib, name)
    words = int(re.search(r"#define\s+HYPEL_COLUMN_RANK_WS_WORDS\s+(\d+)", src).group(1))
    ranks = int(re.search(r"#define\s+HYPEL_COLUMN_RANK_MAX_RANKS\s+(\d+)", src).group(1))
    assert ranks == backend.COLUMN_RANK_MAX_RANKS == 8
    widest = int(re.search(r"#define\s+HYPEL_COLUMN_RANK_MAX_BANDS\s+(\d+)", src).group(1))
    assert widest == backend.COLUMN_RANK_MAX_BANDS == 65536  # 2048 column tiles: inside grid.y
    assert words == backend.COLUMN_RANK_WS_WORDS == 256 + ranks * 256 + ranks * 2


def test_bad_arguments_are_refused_with_a_message(lib):  # noqa: F811
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15  # never dereferenced: every call below fails its argument check first
    ranks = (ctypes.c_int64 * 9)(0, 1, 2, 3, 4, 4, 0, 1, 2)
    r = ctypes.addressof(ranks)
    low = (ctypes.c_int64 * 2)(0, -1)
    high = (ctypes.c_int64 * 2)(0, 5)
    calls = {
        "hypel_band_ratio_f32": [
            (None, 3, p, 3, 5, 3, None, p, 3, p, p), (p, 3, None, 3, 5, 3, None, p, 3, p, p),
            (p, 3, p, 3, 5, 3, None, None, 3, p, p), (p, 3, p, 3, 5, 3, None, p, 3, None, p),
            (p, 3, p, 3, 5, 3, None, p, 3, p, None), (p, 3, p, 3, 0, 3, None, p, 3, p, p),
            (p, 3, p, 3, -5, 3, None, p, 3, p, p), (p, 3, p, 3, 1 << 31, 3, None, p, 3, p, p),
            (p, 3, p, 3, 5, 0, None, p, 3, p, p), (p, 2, p, 3, 5, 3, None, p, 3, p, p),
            (p, 3, p, 2, 5, 3, None, p, 3, p, p), (p, 3, p, 3, 5, 3, None, p, 2, p, p)],
        "hypel_column_rank_select_f32": [
            (None, 3, 5, 3, p, 5, r, 2, p, p), (p, 3, 5, 3, p, 5, None, 2, p, p), (p, 3, 5, 3, p, 5, r, 2, None, p),
            (p, 3, 5, 3, p, 5, r, 2, p, None), (p, 3, 5, 3, p, 5, r, 2, p, p + 4),  # (a misaligned workspace)
            (p, 3, 0, 3, p, 0, r, 2, p, p), (p, 3, -5, 3, p, 5, r, 2, p, p), (p, 3, 1 << 31, 3, p, 5, r, 2, p, p),
            (p, 3, 5, 0, p, 5, r, 2, p, p), (p, 2, 5, 3, p, 5, r, 2, p, p),
            (p, 65537, 5, 65537, p, 5, r, 2, p, p),  # more columns than one call takes
            (p, 3, 5, 3, p, 5, r, 0, p, p), (p, 3, 5, 3, p, 5, r, 9, p, p), (p, 3, 5, 3, p, 5, r, -1, p, p),
            (p, 3, 5, 3, p, 0, r, 1, p, p), (p, 3, 5, 3, p, 6, r, 1, p, p), (p, 3, 5, 3, None, 4, r, 1, p, p),
            (p, 3, 5, 3, p, 4, r, 5, p, p),  # rank 4 of 4 kept rows
            (p, 3, 5, 3, p, 5, ctypes.addressof(low), 2, p, p), (p, 3, 5, 3, p, 5, ctypes.addressof(high), 2, p, p)],
    }
    for name, bad in calls.items():
        fn = getattr(lib, name)
        for args in bad:
            assert fn(*args, None) == -1, (name, args)
            msg = lib.hypel_last_error().decode()
            assert name in msg and "invalid argument" in msg, msg
