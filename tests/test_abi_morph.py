"""CPU: the grey-scale morphology entry points are declared in include/hypel.h, exported by the library and bound from the
header (argument types: tests/test_abi.py, which checks every prototype), and refuse bad arguments with a message before
anything is launched.  New symbols only: the ABI version is still 8 and the header still has 11 structs."""
import ctypes
import re

from tests.test_abi import HEADER, _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_morph_keys_u32", "hypel_morph_erode_dilate_u32", "hypel_morph_reconstruct_sweep_u32",
       "hypel_morph_profile_store_f32")


def names(decl, name):
    return [p[1] for p in decl[name][1]]


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
    assert names(decl, NEW[0]) == ["x", "h", "w", "c", "stride_y", "stride_x", "keys", "stream"]
    assert names(decl, NEW[1]) == ["src", "h", "w", "c", "radius", "shape", "op", "dst", "stream"]
    assert names(decl, NEW[2]) == ["marker_in", "mask", "h", "w", "c", "op", "marker_out", "changed", "stream"]
    assert names(decl, NEW[3]) == ["keys", "h", "w", "c", "pad", "out", "out_c", "chan_offset", "chan_step", "stream"]
    assert backend.MORPH_MAX_RADIUS == abi.const("HYPEL_MORPH_MAX_RADIUS") == 32
    assert (backend.MORPH_MAX_BLOCKS, backend.MORPH_TILE_W, backend.MORPH_TILE_H) == (1024, 64, 16)
    assert (backend.MORPH_DISK, backend.MORPH_SQUARE, backend.MORPH_ERODE, backend.MORPH_DILATE) == (0, 1, 0, 1)


def test_bad_arguments_are_refused_with_a_message(lib):  # noqa: F811
    buf = (ctypes.c_uint8 * (1 << 16))()
    p = ctypes.addressof(buf)  # never dereferenced: every call below fails its argument check first
    q, r, s = p + (1 << 14), p + (2 << 14), p + (3 << 14)
    image = (4, 5, 3)  # h, w, c: 60 elements, 240 bytes
    big = 1 << 31
    calls = {
        "hypel_morph_keys_u32": [
            (None, *image, 15, 3, q), (p, *image, 15, 3, None),
            (p, 0, 5, 3, 15, 3, q), (p, 4, 0, 3, 15, 3, q), (p, -4, 5, 3, 15, 3, q), (p, 4, 5, 0, 15, 3, q),
            (p, 4, 5, -1, 15, 3, q), (p, big, 1, 1, 1, 1, q), (p, 1, big, 1, big, 1, q), (p, 1 << 21, 1 << 21, 1, 1 << 21, 1, q),
            (p, *image, 2, 3, q), (p, *image, 15, 2, q), (p, *image, 15, 0, q), (p, *image, -15, 3, q),  # strides below c
            (p, *image, (1 << 40) + 1, 3, q),
            (p, *image, 15, 3, p), (p, *image, 15, 3, p + 236), (p + 236, *image, 15, 3, p)],  # overlapping ranges
        "hypel_morph_erode_dilate_u32": [
            (None, *image, 1, 0, 0, q), (p, *image, 1, 0, 0, None),
            (p, 0, 5, 3, 1, 0, 0, q), (p, 4, 0, 3, 1, 0, 0, q), (p, 4, 5, 0, 1, 0, 0, q), (p, big, 1, 1, 1, 0, 0, q),
            (p, *image, -1, 0, 0, q), (p, *image, 33, 0, 0, q),  # the radius
            (p, *image, 1, 2, 0, q), (p, *image, 1, -1, 0, q), (p, *image, 1, 0, 2, q), (p, *image, 1, 0, -1, q),  # shape, op
            (p, *image, 1, 0, 0, p), (p, *image, 1, 0, 0, p + 236), (p + 236, *image, 1, 0, 0, p)],
        "hypel_morph_reconstruct_sweep_u32": [
            (None, q, *image, 1, r, s), (p, None, *image, 1, r, s), (p, q, *image, 1, None, s), (p, q, *image, 1, r, None),
            (p, q, 0, 5, 3, 1, r, s), (p, q, 4, 0, 3, 1, r, s), (p, q, 4, 5, 0, 1, r, s), (p, q, big, 1, 1, 1, r, s),
            (p, q, *image, 2, r, s), (p, q, *image, -1, r, s),
            (p, q, *image, 1, p, s), (p, q, *image, 1, q, s), (p, q, *image, 1, p + 236, s), (p, q, *image, 1, q - 236, s),
            (p, q, *image, 1, r, r + 8), (p, q, *image, 1, r, p + 8), (p, q, *image, 1, r, q + 236)],  # the changed word
        "hypel_morph_profile_store_f32": [
            (None, *image, 1, q, 3, 0, 1), (p, *image, 1, None, 3, 0, 1),
            (p, 0, 5, 3, 1, q, 3, 0, 1), (p, 4, 0, 3, 1, q, 3, 0, 1), (p, 4, 5, 0, 1, q, 3, 0, 1),
            (p, *image, -1, q, 3, 0, 1), (p, *image, 5, q, 3, 0, 1), (p, 5, 4, 3, 5, q, 3, 0, 1),  # a pad beyond h or w
            (p, *image, 1, q, 0, 0, 1), (p, *image, 1, q, 3, -1, 1), (p, *image, 1, q, 3, 0, 0), (p, *image, 1, q, 3, 1, 1),
            (p, *image, 1, q, 4, 0, 2), (p, *image, 1, q, 2, 0, 1),  # the last base leaves out_c
            (p, *image, 1, p, 3, 0, 1), (p, *image, 1, p + 236, 3, 0, 1), (p + 500, *image, 1, p, 3, 0, 1)],
    }
    for name, bad in calls.items():
        fn = getattr(lib, name)
        for args in bad:
            assert fn(*args, None) == -1, (name, args)
            msg = lib.hypel_last_error().decode()
            assert name in msg and "invalid argument" in msg, msg
    # what must NOT be refused by these checks is exercised on the device (tests/test_gpu_morph.py): a radius larger
    # than the raster, pad == min(h, w)
