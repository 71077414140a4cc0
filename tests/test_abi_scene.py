"""CPU: the scene-preparation entry points are declared in include/hypel.h, exported by the library (their binding:
tests/test_abi.py, which checks every prototype of the header), and refuse null / negative arguments with a message
before anything is launched.  The ABI version is still 8: new symbols only."""
import ctypes
import re

from tests.test_abi import HEADER, _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_scene_extrema", "hypel_scene_rank_select_u16", "hypel_scene_prepare_f32", "hypel_scene_masked_sums")


def test_version_8_and_new_symbols(lib):  # noqa: F811
    from hypelcnn_amd import backend
    src = open(HEADER).read()
    header = int(re.search(r"#define\s+HYPEL_ABI_VERSION\s+(\d+)", src).group(1))
    assert header == backend.ABI_VERSION == lib.hypel_version() == 8
    decl = _declared()
    for name in NEW:
        assert name in decl and hasattr(lib, name)
    words = int(re.search(r"#define\s+HYPEL_SCENE_RANK_WS_WORDS\s+(\d+)", src).group(1))
    assert words == backend.SCENE_RANK_WS_WORDS == 256 + 2 * 256 + 4


def test_bad_arguments_are_refused_with_a_message(lib):  # noqa: F811
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)  # never dereferenced: every call below fails its argument check first
    geom = (4, 5, 3, 15, 3, 1)
    calls = {
        "hypel_scene_extrema": [
            (None, 1, *geom, None, None, p, p, p, 8), (p, 1, *geom, None, None, None, p, p, 8),
            (p, 1, *geom, None, None, p, p, None, 8), (p, 1, *geom, None, None, p, p, p, 0),
            (p, 1, -4, 5, 3, 15, 3, 1, None, None, p, p, p, 8), (p, 1, 4, 5, 0, 15, 3, 1, None, None, p, p, p, 8),
            (p, 1, 4, 5, 3, -15, 3, 1, None, None, p, p, p, 8), (p, 7, *geom, None, None, p, p, p, 8)],
        "hypel_scene_rank_select_u16": [
            (None, *geom, 0, 1, p, p, p), (p, *geom, 0, 1, None, p, p), (p, *geom, 0, 1, p, p, None),
            (p, *geom, -1, 1, p, p, p), (p, *geom, 2, 1, p, p, p), (p, *geom, 0, 20, p, p, p),
            (p, 4, -5, 3, 15, 3, 1, 0, 1, p, p, p)],
        "hypel_scene_prepare_f32": [
            (None, 1, *geom, 1, None, None, None, p), (p, 1, *geom, 1, None, None, None, None),
            (p, 1, *geom, -1, None, None, None, p), (p, 1, 4, 5, -3, 15, 3, 1, 1, None, None, None, p),
            (p, 9, *geom, 1, None, None, None, p)],
        "hypel_scene_masked_sums": [
            (None, p, 4, 5, 3, p, p, p, 8), (p, None, 4, 5, 3, p, p, p, 8), (p, p, 4, 5, 3, None, p, p, 8),
            (p, p, 4, 5, 3, p, None, p, 8), (p, p, 4, 5, 3, p, p, None, 8), (p, p, -4, 5, 3, p, p, p, 8),
            (p, p, 4, 5, 0, p, p, p, 8), (p, p, 4, 5, 3, p, p, p, -2)],
    }
    for name, bad in calls.items():
        fn = getattr(lib, name)
        for args in bad:
            assert fn(*args, None) == -1, (name, args)
            msg = lib.hypel_last_error().decode()
            assert name in msg and ("invalid argument" in msg or "unsupported" in msg), msg
