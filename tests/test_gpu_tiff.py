"""GPU: csrc/tiff.hip against its NumPy twins (tests/emu_tiff.py) and the golden files, bit for bit -- assemble over
shapes, sample counts, dtypes, byte orders, plane orders, strips and tiles and every predictor, unpack over the golden
streams and the edge streams, malformed streams once the twin has judged the same inputs, and the GRSS2013 / AVON
loaders on rewritten data directories without the scene coming back to the host."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

import tests.emu_tiff as E
from hypelcnn_amd.backend import TIFF_LZW, TIFF_PACKBITS, TIFF_SEG_DTYPE, Ref
from hypelcnn_amd.common import tiff_io as T
from hypelcnn_amd.common.common_nn_ops import SceneArrays, get_loader_from_name
from tests import loader_cases as LC
from tests import tiff_cases as C
from tests.emu_backend import EmuBackend

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_FILES = sorted(glob.glob(os.path.join(GOLDEN, "tiff", "*.tif")))
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def be():
    from hypelcnn_amd.backend import HipBackend
    return HipBackend()


@pytest.fixture(scope="module")
def golden_pixels():
    with np.load(os.path.join(GOLDEN, "tiff", "pixels.npz")) as z:
        return {k: z[k] for k in z.files}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ assemble
def assemble_case(rng, h, w, spp, item, tiled, planar, predictor, swap, from_decoded):
    """random bytes as segments (any bytes are samples), the table, and the call's scalar arguments"""
    seg_rows, seg_cols = (16, 16) if tiled else (5, w)
    across, down = -(-w // seg_cols), -(-h // seg_rows)
    planes = spp if planar == 2 and spp > 1 else 1
    sps = 1 if planes > 1 else spp
    n = planes * across * down
    table = np.zeros(n, TIFF_SEG_DTYPE)
    at = 3  # segments of a file start anywhere: odd offsets, gaps between them
    for i in range(n):
        sy = (i % (across * down)) // across
        rows = seg_rows if tiled else min(seg_rows, h - sy * seg_rows)
        size = rows * seg_cols * sps * item
        table[i] = (at, size, at, size) if from_decoded else (at, size, 0, 0)
        at += size + int(rng.integers(0, 4))
    src = rng.integers(0, 256, at + 5, dtype=np.uint8)
    scalars = (n, int(from_decoded), h, w, spp, item, seg_rows, seg_cols, across, planes, predictor, int(swap))
    return src, table, scalars


def run_assemble(backend, src, table, scalars, out_bytes, pad=64):
    out = backend.upload(np.full(out_bytes + 2 * pad, SENTINEL, np.uint8))
    backend.call("tiff_assemble", Ref(backend.upload(src)), len(src), Ref(backend.upload(table)), *scalars, Ref(out, pad))
    backend.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("item", [1, 2, 4])
@pytest.mark.parametrize("h,w", [(37, 53), (1, 53), (37, 1)])
def test_assemble_against_the_twin(be, h, w, item):
    """item 2 stands for uint16 and int16 alike (the launch moves bits), item 4 for float32"""
    rng = np.random.default_rng(h * 1000 + w * 10 + item)
    emu = EmuBackend()
    n = 0
    for spp in (1, 3, 5, 70):
        for tiled in (False, True):
            for planar in (1, 2):
                for predictor in (1, 2, 3) if item == 4 else (1, 2):
                    for swap in (False, True):
                        case = assemble_case(rng, h, w, spp, item, tiled, planar, predictor, swap, from_decoded=n % 2)
                        want = run_assemble(emu, *case, h * w * spp * item)
                        got = run_assemble(be, *case, h * w * spp * item)
                        assert (want[:64] == SENTINEL).all() and (want[-64:] == SENTINEL).all()
                        assert (want[64:-64] != SENTINEL).any()
                        assert got.tobytes() == want.tobytes(), (spp, tiled, planar, predictor, swap)
                        n += 1
    assert n == (96 if item == 4 else 64)


def test_assemble_leaves_out_rows_its_segment_does_not_hold(be):
    rng = np.random.default_rng(9)
    for spp in (3, 70):
        src, table, scalars = assemble_case(rng, 37, 53, spp, 2, False, 1, 2, False, 0)
        table["src_len"][2] -= 1          # the last row of strip 2 is incomplete
        table["src_off"][5] = len(src) - 7  # strip 5 runs off the buffer
        want = run_assemble(EmuBackend(), src, table, scalars, 37 * 53 * spp * 2)
        got = run_assemble(be, src, table, scalars, 37 * 53 * spp * 2)
        rows = want[64:-64].reshape(37, -1)
        assert (rows[14] == SENTINEL).all() and (rows[25:30] == SENTINEL).all() and not (rows[13] == SENTINEL).all()
        assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ unpack
def run_unpack(backend, streams, needs, codec):
    """segments one behind the other, 8 sentinel bytes around every dst range -> (dst bytes, status, table)"""
    src = np.frombuffer(b"".join(streams), np.uint8)
    t = np.zeros(len(streams), TIFF_SEG_DTYPE)
    at, dst_at = 0, 8
    for i, (s, need) in enumerate(zip(streams, needs)):
        t[i] = (at, len(s), dst_at, need)
        at += len(s)
        dst_at += need + 8
    dst = backend.upload(np.full(dst_at, SENTINEL, np.uint8))
    status = backend.upload(np.full(len(t), -7, np.int32))
    backend.call("tiff_unpack", Ref(backend.upload(src)), len(src), Ref(backend.upload(t)), len(t), codec, Ref(dst),
                 dst_at, Ref(status))
    backend.synchronize()
    return dst.cpu().numpy(), status.cpu().numpy(), t


def golden_streams(codec):
    streams, needs = [], []
    for path in GOLDEN_FILES:
        lay = T.read_layout(path)
        if lay.compression == codec:
            raw = open(path, "rb").read()
            for i in range(lay.n_segments):
                streams.append(raw[lay.offsets[i]:lay.offsets[i] + lay.counts[i]])
                needs.append(lay.segment_bytes(i))
    return streams, needs


def test_unpack_lzw_against_the_twin(be):
    rng = np.random.default_rng(4)
    streams, needs = golden_streams(TIFF_LZW)  # the table-reset stream among them
    assert len(streams) == 4 * 8 + 4 + 1 + 1 and max(needs) == 96 * 96 * 2
    row = bytes(rng.integers(0, 3, 53, dtype=np.uint8))
    extra = [(b"\x2a", 1), (b"\x00" * 5000, 5000)]                  # 1 byte; long self-overlapping copies
    extra += [(bytes(rng.integers(0, 256, n, dtype=np.uint8)), n) for n in (7, 8, 9, 15, 16)]  # ends on / off a byte
    for data, need in extra:
        streams.append(C.lzw_encode(data))
        needs.append(need)
    block = bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    far = block + b"\x00" * 40000 + block     # strings of the first block, used again 40000 bytes later
    extra.append((far, len(far)))
    for data, need in extra[-1:]:
        streams.append(C.lzw_encode(data))
        needs.append(need)
    text = b"abcabcabcabc" * 20
    streams.append(C.lzw_encode(text)[:-2])   # no EOI: dst_len is reached first
    needs.append(len(text) - 9)
    streams += [C.lzw_encode(bytes((b + i) & 255 for b in row)) for i in range(300)]  # 300 one-row segments
    needs += [53] * 300
    want, want_st, _ = run_unpack(EmuBackend(), streams, needs, TIFF_LZW)
    got, got_st, t = run_unpack(be, streams, needs, TIFF_LZW)
    assert (want_st == 0).all()
    assert got_st.tolist() == want_st.tolist() and got.tobytes() == want.tobytes()
    k = len(streams) - 300 - 1 - len(extra)
    lo = int(t["dst_off"][k + 1])
    assert got[lo:lo + 5000].tobytes() == b"\x00" * 5000 and (got[lo + 5000:lo + 5008] == SENTINEL).all()


def test_unpack_packbits_against_the_twin(be):
    streams, needs = golden_streams(TIFF_PACKBITS)
    assert len(streams) == 5 * 8
    lit = bytes(range(128))
    streams += [bytes([127]) + lit, bytes([129, 7]), bytes([128, 128, 2, 1, 2, 3]), bytes([200, 9]), bytes([0, 77])]
    needs += [128, 128, 3, 20, 1]  # 128 literals; 128 repeats; the -128 no-op; a run clipped at dst_len; one byte
    row = np.repeat(np.arange(18, dtype=np.uint8), 3)
    streams += [C.packbits_encode(bytes(row + np.uint8(i % 200))) for i in range(300)]
    needs += [54] * 300
    want, want_st, _ = run_unpack(EmuBackend(), streams, needs, TIFF_PACKBITS)
    got, got_st, _ = run_unpack(be, streams, needs, TIFF_PACKBITS)
    assert (want_st == 0).all()
    assert got_st.tolist() == want_st.tolist() and got.tobytes() == want.tobytes()


def test_malformed_streams_get_a_status_and_touch_nothing_else(be):
    """Ordinary data to a decoder whose reads and writes are bounded.  Should either fault, a bound is missing: to be
    found by reading the kernel against the twin."""
    from tests.test_tiff_emu import pack_codes
    text = bytes(np.random.default_rng(1).integers(0, 4, 400, dtype=np.uint8))
    good = C.lzw_encode(b"neighbour" * 9)
    above = pack_codes([(256, 9), (65, 9), (66, 9), (300, 9), (257, 9)])
    cut = C.lzw_encode(text)[:60]
    streams, needs = [good, above, good, cut, good], [81, 16, 81, 400, 81]
    want, want_st, t = run_unpack(EmuBackend(), streams, needs, TIFF_LZW)
    assert want_st.tolist() == [0, E.BAD_CODE, 0, E.TRUNCATED, 0]  # the twin first
    got, got_st, _ = run_unpack(be, streams, needs, TIFF_LZW)
    assert got_st.tolist() == want_st.tolist()
    covered = np.zeros(got.size, bool)
    for i, rec in enumerate(t):
        lo, hi = int(rec["dst_off"]), int(rec["dst_off"] + rec["dst_len"])
        covered[lo:hi] = True
        if got_st[i] == 0:
            assert got[lo:hi].tobytes() == b"neighbour" * 9
    assert (got[~covered] == SENTINEL).all()
    assert got.tobytes() == want.tobytes()  # what was decoded in front of the fault included
    pb = [C.packbits_encode(b"neighbour" * 9), bytes([5, 1, 2]), C.packbits_encode(b"neighbour" * 9)]
    want, want_st, _ = run_unpack(EmuBackend(), pb, [81, 6, 81], TIFF_PACKBITS)
    assert want_st.tolist() == [0, E.TRUNCATED, 0]
    got, got_st, _ = run_unpack(be, pb, [81, 6, 81], TIFF_PACKBITS)
    assert got_st.tolist() == want_st.tolist() and got.tobytes() == want.tobytes()
    # the process goes on: a read through the whole path still works
    path = os.path.join(GOLDEN, "tiff", "lzw_2_I16.tif")
    assert same(T.read_raster(path, be).download(), T.imread(path))


# ------------------------------------------------------------------------------------------------ files
def test_read_raster_reads_the_goldens(be, golden_pixels):
    for path in GOLDEN_FILES:
        stem = os.path.basename(path)[:-4]
        got = T.read_raster(path, be)
        assert got.bytes.is_cuda
        assert same(got.download(), golden_pixels["reset" if "reset" in stem else stem.split("_")[-1]]), stem


def test_read_raster_reads_written_variants(be, tmp_path):
    rng = np.random.default_rng(5)
    for spp, dtype in ((5, np.int16), (70, np.uint16), (1, np.float32)):
        a = rng.integers(-3000, 3000, (37, 53, spp)).astype(dtype)
        for i, kw in enumerate((dict(tile=C.TILE, compression=C.LZW, predictor=2, order=">"),
                                dict(rows_per_strip=5, planar=2, compression=C.DEFLATE, predictor=3 if spp == 1 else 2),
                                dict(tile=C.TILE, planar=2, compression=C.PACKBITS), dict(rows_per_strip=1, order=">"))):
            p = str(tmp_path / f"m{spp}_{i}.tif")
            C.write_tiff(p, a, **kw)
            assert same(T.read_raster(p, be).download(), a.reshape(T.read_layout(p).shape)), (spp, kw)


def test_a_bad_stream_in_a_file_names_its_segment(be, tmp_path):
    p = str(tmp_path / "cut.tif")
    C.write_tiff(p, C.pixels("u16"), rows_per_strip=5, compression=C.LZW)
    lay = T.read_layout(p)
    raw = bytearray(open(p, "rb").read())
    at = lay.offsets[3]
    raw[at:at + 4] = C.lzw_encode(b"ab")[:4]  # a valid, far too short stream where strip 3 began: EOI after 2 bytes
    open(p, "wb").write(raw)
    with pytest.raises(ValueError, match="segment 3"):
        T.read_raster(p, be)
    with pytest.raises(ValueError, match="segment 3"):
        T.imread(p)


# ------------------------------------------------------------------------------------------------ loaders
@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "reference_loaders.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def rewritten(tmp_path_factory):
    base = LC.write_data_dir(str(tmp_path_factory.mktemp("loader_data")))
    return {how: C.rewrite_scenes(shutil.copytree(base, str(tmp_path_factory.mktemp("rewritten") / how)), how)
            for how in ("tiles", "strips")}


@pytest.mark.parametrize("how", ["tiles", "strips"])
@pytest.mark.parametrize("name,case,attrs", [("GRSS2013DataLoader", "normalized", {}), ("AVONDataLoader", "normalized", {}),
                                             ("AVONDataLoader", "shcorrected", {"load_shadow_corrected": True})])
def test_loaders_on_rewritten_directories(be, gold, rewritten, name, case, attrs, how):
    loader = get_loader_from_name(name, rewritten[how])  # no backend given: the visible HIP device is used
    for k, v in attrs.items():
        setattr(loader, k, v)
    ds = loader.load_data(LC.NEIGHBORHOOD, True)
    assert type(ds).__name__ == "DeviceBasicDataSet" and ds.casi_dev.is_cuda
    key = f"{name}/{case}"
    for what in ("casi_min", "casi_max", "lidar_min", "lidar_max"):
        got, want = np.asarray(getattr(ds, what)), gold[f"{key}/{what}"]
        assert got.dtype == want.dtype and np.array_equal(got, want), what
    targets = np.asarray([(x, y, 0) for x, y in LC.POINTS])
    arrays = SceneArrays()
    arrays.feed(ds, targets, be)
    out, _ = arrays.gather(torch.arange(len(targets), device=be.device))
    want = gold[f"{key}/patches"].astype(np.float32)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert ds.downloaded() == []


@pytest.mark.parametrize("how", ["tiles", "strips"])
def test_grss2018_decodes_on_the_device(be, tmp_path, how):
    """its data set is prepared on the host, from rasters the device decoded"""
    from hypelcnn_amd.loader.GRSS2018DataLoader import GRSS2018DataLoader, GRSS2018DataSet
    base = C.rewrite_scenes(C.write_grss2018_dir(str(tmp_path)), how)
    casi, lidar = C.grss2018_pixels()
    lidar = lidar[:, :, None].copy()
    lidar[lidar > 300] = 0
    want = GRSS2018DataSet(shadow_creator_dict=None, casi=casi[:, :, :-2], lidar=lidar, neighborhood=2, normalize=True)
    seen = []
    real = be.call
    be.call = lambda name, *a: (seen.append(name), real(name, *a))[1]
    try:
        loader = GRSS2018DataLoader(base)
        loader.backend = be  # (the one whose calls are watched; without it the visible HIP device is used just so)
        ds = loader.load_data(2, True)
    finally:
        del be.call
    assert [n for n in seen if n.startswith("tiff")] == (["tiff_unpack", "tiff_assemble"] if how == "tiles" else ["tiff_assemble"]) * 2
    for what in ("casi", "lidar", "casi_max", "lidar_max"):
        assert same(getattr(ds, what), getattr(want, what)), what
    assert same(ds.get_data_point(5, 7), want.get_data_point(5, 7))


def test_avon_scene_of_another_dtype(be, gold, rewritten, tmp_path):
    base = shutil.copytree(rewritten["strips"], str(tmp_path / "int16"))
    path = base + "/AVON/0920-1857.georef_cropped.tif"
    C.write_tiff(path, T.imread(path).view(np.int16), tile=C.TILE, compression=C.LZW, predictor=2)
    ds = get_loader_from_name("AVONDataLoader", base).load_data(LC.NEIGHBORHOOD, True)
    assert type(ds).__name__ == "DeviceBasicDataSet"
    assert np.array_equal(np.asarray(ds.casi_max), gold["AVONDataLoader/normalized/casi_max"])
    targets = np.asarray([(x, y, 0) for x, y in LC.POINTS])
    arrays = SceneArrays()
    arrays.feed(ds, targets, be)
    out, _ = arrays.gather(torch.arange(len(targets), device=be.device))
    want = gold["AVONDataLoader/normalized/patches"].astype(np.float32)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
