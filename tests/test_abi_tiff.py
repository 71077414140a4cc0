"""CPU: the two TIFF entry points are declared in include/hypel.h, exported by the library (their binding:
tests/test_abi.py, which checks every prototype of the header), and refuse bad scalar arguments with a message before
anything is launched (there is no device here: a launch would fail with another code).  The ABI version is still 8."""
import ctypes
import re

from tests.test_abi import HEADER, _declared, lib  # noqa: F401 -- `lib` is the module fixture of tests/test_abi.py

NEW = ("hypel_tiff_unpack", "hypel_tiff_assemble")


def test_version_8_and_new_symbols(lib):  # noqa: F811
    from hypelcnn_amd import backend
    src = open(HEADER).read()
    header = int(re.search(r"#define\s+HYPEL_ABI_VERSION\s+(\d+)", src).group(1))
    assert header == backend.ABI_VERSION == lib.hypel_version() == 8
    decl = _declared()
    for name in NEW:
        assert name in decl and hasattr(lib, name)
    assert backend.TIFF_SEG_DTYPE.itemsize == 32 and backend.TIFF_SEG_DTYPE.names == ("src_off", "src_len", "dst_off", "dst_len")
    assert [backend.TIFF_SEG_DTYPE.fields[n][1] for n in backend.TIFF_SEG_DTYPE.names] == [0, 8, 16, 24]
    codes = dict(re.findall(r"HYPEL_TIFF_(LZW|PACKBITS)\s*=\s*(\d+)", src))
    assert (int(codes["LZW"]), int(codes["PACKBITS"])) == (backend.TIFF_LZW, backend.TIFF_PACKBITS) == (5, 32773)


def test_bad_arguments_are_refused_with_a_message(lib):  # noqa: F811
    for name in NEW:
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)  # never dereferenced: every call below fails its argument check first
    # assemble: src, src_bytes, segs, n_segs, from_decoded, h, w, spp, item, seg_rows, seg_cols, segs_across, planes,
    # predictor, swap, out -- a valid call is 37 x 53 x 3 uint16 in 16 x 16 tiles: 4 across, 3 down
    good = [p, 4096, p, 12, 1, 37, 53, 3, 2, 16, 16, 4, 1, 1, 0, p]

    def but(**kw):
        names = ["src", "src_bytes", "segs", "n_segs", "from_decoded", "h", "w", "spp", "item", "seg_rows", "seg_cols",
                 "segs_across", "planes", "predictor", "swap", "out"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return tuple(a)

    calls = {
        "hypel_tiff_unpack": [
            (None, 64, p, 1, 5, p, 64, p), (p, 64, None, 1, 5, p, 64, p), (p, 64, p, 1, 5, None, 64, p),
            (p, 64, p, 1, 5, p, 64, None), (p, 0, p, 1, 5, p, 64, p), (p, 64, p, 0, 5, p, 64, p),
            (p, 64, p, -3, 32773, p, 64, p), (p, 64, p, 1, 5, p, -1, p), (p, 64, p, 1, 8, p, 64, p),
            (p, 64, p, 1, 0, p, 64, p)],
        "hypel_tiff_assemble": [
            but(src=None), but(segs=None), but(out=None), but(src_bytes=0), but(n_segs=0), but(n_segs=11),
            but(h=0), but(w=-53), but(spp=0), but(item=3), but(item=8), but(seg_rows=0), but(seg_cols=-16),
            but(segs_across=3), but(planes=2), but(planes=3, n_segs=12), but(predictor=0), but(predictor=4),
            but(predictor=3), but(from_decoded=2), but(swap=-1), but(out=p + 1)],
    }
    for name, bad in calls.items():
        fn = getattr(lib, name)
        for args in bad:
            assert fn(*args, None) == -1, (name, args)
            msg = lib.hypel_last_error().decode()
            assert name in msg and "invalid argument" in msg, msg
