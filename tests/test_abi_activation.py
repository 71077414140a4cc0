"""CPU: the activation entry points are declared in include/hypel.h, exported by the library and bound from the header
(argument types: tests/test_abi.py, which checks every prototype), refuse bad arguments with a message before anything
is launched, and launch nothing for a view of no rows.  New symbols only: the ABI version is still 8 and the header
still has 11 structs."""
import ctypes
import re

from tests.test_abi import HEADER, _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_view_range_f32", "hypel_view_histogram_f32")


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
    assert backend.ACT_MAX_BINS == abi.const("HYPEL_ACT_MAX_BINS") == 4096
    assert [p[1] for p in decl["hypel_view_range_f32"][1]] == ["src", "rows", "ld", "cols", "range", "count", "stream"]
    assert [p[1] for p in decl["hypel_view_histogram_f32"][1]] == ["src", "rows", "ld", "cols", "edges", "n_bins",
                                                                   "counts", "outside", "stream"]
    assert [p[0] for p in decl["hypel_view_histogram_f32"][1][1:4]] == ["int64_t", "int64_t", "int32_t"]


def test_bad_arguments_are_refused_with_a_message(lib):  # noqa: F811
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)  # never dereferenced: every call below fails its argument check first
    q, r, s = p + 1024, p + 2048, p + 3072
    views = [(-1, 8, 8), (4, 8, 0), (4, 8, -3), (4, 7, 8), (4, -8, 8),  # rows < 0, cols < 1, ld < cols
             (1 << 36, 2, 2), (1 << 30, 128, 128), ((1 << 37) - 1, 2, 2),  # 2^37 elements or more
             (1 << 30, 1 << 33, 1)]  # rows * ld beyond 2^62
    calls = {
        "hypel_view_range_f32": [(None, 4, 8, 8, q, r), (p, 4, 8, 8, None, r), (p, 4, 8, 8, q, None)] +
                                [(p, *v, q, r) for v in views],
        "hypel_view_histogram_f32": [(None, 4, 8, 8, q, 4, r, s), (p, 4, 8, 8, None, 4, r, s), (p, 4, 8, 8, q, 4, None, s),
                                     (p, 4, 8, 8, q, 4, r, None), (p, 4, 8, 8, q, 0, r, s), (p, 4, 8, 8, q, -1, r, s),
                                     (p, 4, 8, 8, q, 4097, r, s), (p, 0, 8, 8, q, 4097, r, s)] +
                                    [(p, *v, q, 4, r, s) for v in views],
    }
    for name, bad in calls.items():
        fn = getattr(lib, name)
        for args in bad:
            assert fn(*args, None) == -1, (name, args)
            msg = lib.hypel_last_error().decode()
            assert name in msg and "invalid argument" in msg, msg


def test_a_view_of_no_rows_launches_nothing(lib):  # noqa: F811
    """rows == 0 is answered on the host: OK, and the outputs (host memory here, never touched) keep their values"""
    src = (ctypes.c_float * 8)(*[1.0] * 8)
    rng = (ctypes.c_float * 2)(3.0e38, -3.0e38)
    count = (ctypes.c_int64 * 2)(5, 6)
    edges = (ctypes.c_double * 3)(0.0, 1.0, 2.0)
    counts = (ctypes.c_int64 * 2)(7, 8)
    outside = (ctypes.c_int64 * 1)(9)
    a = ctypes.addressof
    assert lib.hypel_view_range_f32(a(src), 0, 8, 8, a(rng), a(count), None) == 0
    assert lib.hypel_view_histogram_f32(a(src), 0, 8, 8, a(edges), 2, a(counts), a(outside), None) == 0
    assert list(rng) == [ctypes.c_float(3.0e38).value, ctypes.c_float(-3.0e38).value]
    assert (list(count), list(counts), list(outside)) == ([5, 6], [7, 8], [9])
