"""CPU: the band-PCA entry points are declared in include/hypel.h, exported by the library and bound from the header
(argument types: tests/test_abi.py, which checks every prototype), and refuse bad arguments with a message before
anything is launched.  New symbols only: the ABI version is still 8 and the header still has 11 structs."""
import ctypes
import re

from tests.test_abi import HEADER, _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_pca_band_sums_f64", "hypel_pca_scatter_f64", "hypel_pca_project_f32")


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
        assert [p[1] for p in params[:6]] == ["x", "h", "w", "c", "stride_y", "stride_x"]
    assert (backend.PCA_MAX_BANDS, backend.PCA_CHUNK, backend.PCA_TILE, backend.PCA_MAX_BLOCKS) == (512, 1024, 64, 1024)
    assert abi.const("HYPEL_PCA_PROJECT_MAX_BLOCKS") == 4096
    assert [p[1] for p in decl["hypel_pca_project_f32"][1][6:12]] == ["pass", "mean", "weights", "k", "out", "ldo"]


def test_workspace_formulas():
    from hypelcnn_amd.classic.decomposition import band_sums_ws_doubles, scatter_ws_doubles
    assert band_sums_ws_doubles(1, 3) == 3 and band_sums_ws_doubles(1025, 3) == 6
    assert band_sums_ws_doubles(1 << 30, 512) == 1024 * 512
    assert scatter_ws_doubles(1, 3) == 4096 and scatter_ws_doubles(5000, 64) == 5 * 4096
    assert scatter_ws_doubles(5000, 65) == 5 * 3 * 4096 and scatter_ws_doubles(1 << 30, 144) == 170 * 6 * 4096
    assert scatter_ws_doubles(1 << 30, 512) == 28 * 36 * 4096 <= 1024 * 4096


def test_bad_arguments_are_refused_with_a_message(lib):  # noqa: F811
    buf = (ctypes.c_uint8 * (1 << 16))()
    p = ctypes.addressof(buf)  # never dereferenced: every call below fails its argument check first
    q, r, s = p + (1 << 14), p + (2 << 14), p + (3 << 14)
    view = (4, 5, 3, 15, 3)  # h, w, c, stride_y, stride_x: 20 pixels, 60 floats
    ws = 1 << 20
    calls = {
        "hypel_pca_band_sums_f64": [
            (None, *view, q, r, ws), (p, *view, None, r, ws), (p, *view, q, None, ws), (p, *view, q, q, ws),
            (p, 0, 5, 3, 15, 3, q, r, ws), (p, 4, 0, 3, 15, 3, q, r, ws), (p, -4, 5, 3, 15, 3, q, r, ws),
            (p, 4, 5, 0, 15, 3, q, r, ws), (p, 4, 5, 513, 5 * 513, 513, q, r, ws), (p, 4, 5, -1, 15, 3, q, r, ws),
            (p, 4, 5, 3, 2, 3, q, r, ws), (p, 4, 5, 3, 15, 2, q, r, ws), (p, 4, 5, 3, 15, 0, q, r, ws),  # strides below c
            (p, 4, 5, 3, -15, 3, q, r, ws), (p, (1 << 40) + 1, 1, 3, 3, 3, q, r, ws), (p, 1 << 21, 1 << 21, 3, 3, 3, q, r, ws),
            (p, *view, q, r, 2), (p, *view, q, r, 0), (p, *view, q, r, -1),  # a short workspace: 1 block * 3 bands
            (p, 1, 1025, 3, 3075, 3, q, r, 5),  # ... two chunks
            (p, *view, p + 8, r, ws), (p, *view, q, p + 16, ws), (p, *view, q, q + 8, ws)],  # overlapping ranges
        "hypel_pca_scatter_f64": [
            (None, *view, q, r, s, ws), (p, *view, None, r, s, ws), (p, *view, q, None, s, ws), (p, *view, q, r, None, ws),
            (p, *view, q, r, r, ws),
            (p, 0, 5, 3, 15, 3, q, r, s, ws), (p, 4, 0, 3, 15, 3, q, r, s, ws), (p, 4, 5, 0, 15, 3, q, r, s, ws),
            (p, 4, 5, 513, 5 * 513, 513, q, r, s, ws), (p, 4, 5, 3, 2, 3, q, r, s, ws), (p, 4, 5, 3, 15, 2, q, r, s, ws),
            (p, 1 << 21, 1 << 21, 3, 3, 3, q, r, s, ws),
            (p, *view, q, r, s, 4095), (p, *view, q, r, s, 0),  # a short workspace: one tile of one group
            (p, 4, 5, 65, 5 * 65, 65, q, r, s, 3 * 4096 - 1),  # ... three tiles
            (p, 1, 1025, 3, 3075, 3, q, r, s, 2 * 4096 - 1),  # ... two groups
            (p, *view, q, p + 64, s, ws), (p, *view, q, r, p + 128, ws), (p, *view, q, q, s, ws), (p, *view, q, r, q, ws),
            (p, *view, q, r, r + 8, ws)],
        "hypel_pca_project_f32": [
            (None, *view, 0, q, r, 2, s, 2), (p, *view, 0, None, r, 2, s, 2), (p, *view, 0, q, None, 2, s, 2),
            (p, *view, 0, q, r, 2, None, 2),
            (p, 0, 5, 3, 15, 3, 0, q, r, 2, s, 2), (p, 4, 5, 0, 15, 3, 0, q, r, 1, s, 2),
            (p, 4, 5, 513, 5 * 513, 513, 0, q, r, 2, s, 2), (p, 4, 5, 3, 2, 3, 0, q, r, 2, s, 2),
            (p, 4, 5, 3, 15, 2, 0, q, r, 2, s, 2),
            (p, *view, 0, q, r, 4, s, 4), (p, *view, 0, q, r, 0, s, 2), (p, *view, 0, q, r, -1, s, 2),  # k > c, k < 1
            (p, *view, -1, q, r, 2, s, 2), (p, *view, 1, q, r, 2, s, 3),  # pass < 0; strides below c + pass
            (p, 4, 5, 3, 20, 4, 1, q, r, 2, s, 2), (p, 4, 5, 3, 20, 4, 1, q, r, 3, s, 3),  # ldo < k + pass
            (p, *view, 0, q, r, 2, s, 1), (p, *view, 0, q, r, 2, s, 0), (p, *view, 0, q, r, 2, s, -2),
            (p, *view, 0, q, r, 2, p, 2), (p, *view, 0, q, r, 2, p + 236, 2), (p + 156, *view, 0, q, r, 2, p, 2),  # overlap
            (p, *view, 0, q, r, 2, q, 2), (p, *view, 0, q, r, 2, r + 20, 2)],  # the mean, the weights
    }
    for name, bad in calls.items():
        fn = getattr(lib, name)
        for args in bad:
            assert fn(*args, None) == -1, (name, args)
            msg = lib.hypel_last_error().decode()
            assert name in msg and "invalid argument" in msg, msg
