"""CPU: the template-matching entry points are declared in include/hypel.h, exported by the library and bound from the
header (argument types: tests/test_abi.py, which checks every prototype), and refuse bad arguments with a message before
anything is launched.  New symbols only: the ABI version is still 8 and the header still has 11 structs."""
import ctypes
import re

from tests.test_abi import HEADER, _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_match_ccorr_f32", "hypel_match_window_energy_f64", "hypel_match_best_f32", "hypel_match_render_u8")


def test_version_8_eleven_structs_and_new_symbols(lib):  # noqa: F811
    from hypelcnn_amd import abi, backend
    src = open(HEADER).read()
    header = int(re.search(r"#define\s+HYPEL_ABI_VERSION\s+(\d+)", src).group(1))
    assert header == backend.ABI_VERSION == lib.hypel_version() == 8
    assert len(abi.STRUCTS) == 11
    decl = _declared()
    for name in NEW:
        assert name in decl and hasattr(lib, name)
        params = decl[name][1]
        assert params[-1][:2] == ("hypel_stream_t", "stream")
        assert getattr(lib, name).argtypes == [kind for _, _, kind in params]
        assert name[len("hypel_"):] in backend.SIGNATURES
    assert (backend.MATCH_TILE, backend.MATCH_ROW_CHUNK, backend.MATCH_COL_CHUNK) == (16, 32, 32)
    assert backend.MATCH_BLOCK_COLS == 128 and backend.MATCH_MAX_SPLITS == 4096
    assert [p[1] for p in decl["hypel_match_ccorr_f32"][1][:6]] == ["image", "h", "w", "sy", "sx", "scale"]
    assert [p[1] for p in decl["hypel_match_ccorr_f32"][1][6:12]] == ["tmpl", "ht", "wt", "tsy", "tsx", "tscale"]
    assert decl["hypel_match_best_f32"][1][6][:2] == ("void*", "result")


def test_bad_arguments_are_refused_with_a_message(lib):  # noqa: F811
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)  # never dereferenced: every call below fails its argument check first
    q, r, s = p + 1024, p + 2048, p + 3072
    img, tpl = (6, 8, 8, 1, 1), (3, 4, 4, 1, 1)  # h, w, sy, sx, scale
    calls = {
        "hypel_match_ccorr_f32": [
            (None, *img, q, *tpl, r, None, 1), (p, *img, None, *tpl, r, None, 1), (p, *img, q, *tpl, None, None, 1),
            (p, *img, q, *tpl, p, None, 1), (p, *img, q, *tpl, q, None, 1),  # num aliases an input
            (p, 0, 8, 8, 1, 1, q, *tpl, r, None, 1), (p, 6, -8, 8, 1, 1, q, *tpl, r, None, 1),
            (p, *img, q, 0, 4, 4, 1, 1, r, None, 1), (p, *img, q, 3, 0, 4, 1, 1, r, None, 1),
            (p, 6, 8, -8, 1, 1, q, *tpl, r, None, 1), (p, *img, q, 3, 4, 4, -1, 1, r, None, 1),
            (p, 6, 8, 8, 1, 0, q, *tpl, r, None, 1), (p, *img, q, 3, 4, 4, 1, 0, r, None, 1),  # scales below 1
            (p, 6, 8, 8, 1, -2, q, *tpl, r, None, 1),
            (p, *img, q, 7, 4, 4, 1, 1, r, None, 1), (p, *img, q, 3, 9, 9, 1, 1, r, None, 1),  # template larger
            (p, *img, q, 3, 4, 4, 1, 3, r, None, 1),  # ... once enlarged: 9 rows over 6
            (p, 1 << 16, 1 << 15, 1 << 15, 1, 1, q, *tpl, r, None, 1),  # 2^31 pixels
            (p, 1 << 14, 1 << 13, 1 << 13, 1, 4, q, *tpl, r, None, 1),  # ... once enlarged
            (p, *img, q, *tpl, r, None, 0), (p, *img, q, *tpl, r, None, 4097), (p, *img, q, *tpl, r, None, -1),
            (p, *img, q, *tpl, r, None, 2), (p, *img, q, *tpl, r, r, 2), (p, *img, q, *tpl, r, p, 2),  # ws null / aliased
            (p, 30000, 30000, 30000, 1, 1, q, 1, 1, 1, 1, 1, r, s, 3)],  # partial surfaces reach 2^31
        "hypel_match_window_energy_f64": [
            (None, *img, 3, 4, q, r), (p, *img, 3, 4, None, r), (p, *img, 3, 4, q, None), (p, *img, 3, 4, q, q),
            (p, *img, 3, 4, p, r), (p, *img, 3, 4, q, p),
            (p, 0, 8, 8, 1, 1, 3, 4, q, r), (p, 6, 0, 8, 1, 1, 3, 4, q, r), (p, 6, 8, 8, 1, 0, 3, 4, q, r),
            (p, 6, 8, -1, 1, 1, 3, 4, q, r), (p, *img, 0, 4, q, r), (p, *img, 3, 0, q, r), (p, *img, 7, 4, q, r),
            (p, *img, 3, 9, q, r), (p, 1 << 16, 1 << 15, 1 << 15, 1, 1, 3, 4, q, r)],
        "hypel_match_best_f32": [
            (None, q, r, 4, 5, None, s), (p, None, r, 4, 5, None, s), (p, q, None, 4, 5, None, s),
            (p, q, r, 4, 5, None, None), (p, q, r, 4, 5, p, s), (p, q, r, 4, 5, s, s), (p, q, r, 4, 5, None, p),
            (p, q, r, 4, 5, None, q), (p, q, r, 4, 5, None, r),
            (p, q, r, 0, 5, None, s), (p, q, r, 4, -5, None, s), (p, q, r, 1 << 16, 1 << 15, None, s),
            (p, q, r, 4, 5, None, s + 4)],  # the record is 8-byte aligned
        "hypel_match_render_u8": [
            (None, *img, q, r), (p, *img, None, r), (p, *img, q, None), (p, *img, q, p), (p, *img, q, q),
            (p, 0, 8, 8, 1, 1, q, r), (p, 6, 8, 8, 1, 0, q, r), (p, 6, 8, 8, -1, 1, q, r),
            (p, 1 << 14, 1 << 13, 1 << 13, 1, 4, q, r)],
    }
    for name, bad in calls.items():
        fn = getattr(lib, name)
        for args in bad:
            assert fn(*args, None) == -1, (name, args)
            msg = lib.hypel_last_error().decode()
            assert name in msg and "invalid argument" in msg, msg
