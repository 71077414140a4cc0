"""CPU: the shadow-region entry points are declared in include/hypel.h, exported by the library and bound from the
header (argument types: tests/test_abi.py, which checks every prototype), and refuse bad arguments with a message before
anything is launched.  New symbols only: the ABI version is still 8 and the header still has 11 structs."""
import ctypes
import re

from tests.test_abi import HEADER, _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_components_label_u8", "hypel_components_compact_i32", "hypel_components_votes_i32",
       "hypel_components_relabel_u8", "hypel_shadow_correct_f32")


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
    assert backend.COMPONENTS_MAX_CLASSES == 64 and backend.COMPONENTS_OK == 0 and backend.COMPONENTS_STEP_CAP == 1
    assert decl["hypel_components_votes_i32"][1][6][:2] == ("uint64_t", "exclude")


def test_bad_arguments_are_refused_with_a_message(lib):  # noqa: F811
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)  # never dereferenced: every call below fails its argument check first
    q = p + 1024
    geom = (15, 3, 1)  # element strides of a [4][5][3] raster
    calls = {
        "hypel_components_label_u8": [
            (None, 4, 5, p, q, p), (p, 4, 5, None, q, p), (p, 4, 5, p, None, p), (p, 4, 5, p, q, None),
            (p, 4, 5, p, p, p), (p, 0, 5, p, q, p), (p, 4, 0, p, q, p), (p, -4, 5, p, q, p), (p, 4, -5, p, q, p),
            (p, 1 << 16, 1 << 15, p, q, p)],
        "hypel_components_compact_i32": [
            (None, 4, 5, q, p, p), (p, 4, 5, None, p, p), (p, 4, 5, q, None, p), (p, 4, 5, q, p, None),
            (p, 4, 5, p, p, p), (p, 0, 5, q, p, p), (p, 4, -1, q, p, p), (p, 1 << 16, 1 << 15, q, p, p)],
        "hypel_components_votes_i32": [
            (None, p, 4, 5, 2, 11, 0, p, p, p), (p, None, 4, 5, 2, 11, 0, p, p, p), (p, p, 4, 5, 2, 11, 0, None, p, p),
            (p, p, 4, 5, 2, 11, 0, p, None, p), (p, p, 4, 5, 2, 11, 0, p, p, None), (p, p, 0, 5, 2, 11, 0, p, p, p),
            (p, p, 4, -5, 2, 11, 0, p, p, p), (p, p, 4, 5, -1, 11, 0, p, p, p), (p, p, 4, 5, 21, 11, 0, p, p, p),
            (p, p, 4, 5, 2, 0, 0, p, p, p), (p, p, 4, 5, 2, 65, 0, p, p, p), (p, p, 4, 5, 2, -3, 0, p, p, p)],
        "hypel_components_relabel_u8": [
            (None, p, p, 4, 5, 0, q), (p, None, p, 4, 5, 0, q), (p, p, None, 4, 5, 0, q), (p, p, p, 4, 5, 1, None),
            (p, p, p, 0, 5, 0, q), (p, p, p, 4, 0, 0, q)],
        "hypel_shadow_correct_f32": [
            (None, 0, 4, 5, 3, *geom, p, p, q), (p, 0, 4, 5, 3, *geom, None, p, q), (p, 0, 4, 5, 3, *geom, p, None, q),
            (p, 0, 4, 5, 3, *geom, p, p, None), (p, 0, 4, 5, 3, *geom, p, p, p), (p, 0, 0, 5, 3, *geom, p, p, q),
            (p, 0, 4, -5, 3, *geom, p, p, q), (p, 0, 4, 5, 0, *geom, p, p, q), (p, 0, 4, 5, 3, -15, 3, 1, p, p, q),
            (p, 9, 4, 5, 3, *geom, p, p, q)],
    }
    for name, bad in calls.items():
        fn = getattr(lib, name)
        for args in bad:
            assert fn(*args, None) == -1, (name, args)
            msg = lib.hypel_last_error().decode()
            assert name in msg and ("invalid argument" in msg or "unsupported" in msg), msg
