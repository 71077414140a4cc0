"""TEST INFRASTRUCTURE: a TIFF writer for the layouts PIL cannot write -- tiles, planes, big-endian files, any of
them compressed -- with its own straightforward LZW and PackBits encoders, written from the TIFF 6.0 text and
independent of the decoders under test.  Where PIL imports, tests/test_tiff_emu.py makes PIL read every variant listed
here back to the written pixels (big-endian float32 excepted by name: PIL returns its values unswapped)."""
import hashlib
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

H, W = 37, 53          # with 16 x 16 tiles and 5 rows per strip neither divides: edge tiles both ways, a 2-row strip
TILE, ROWS = (16, 16), 5
NONE, LZW, DEFLATE, PACKBITS = 1, 5, 8, 32773


def lzw_encode(data):
    """TIFF LZW: MSB-first codes, Clear first, 9 bits growing to 12 one code early, Clear again before the table is
    full, EOI last.  Strings are keyed (prefix code << 8 | byte)."""
    out = bytearray()
    acc = nacc = 0
    table, free, codes, w = {}, 258, 0, -1

    def emit(code):
        """at the width the reader expects once `codes` codes followed the last Clear: it has 257 + codes entries
        then, and widens one entry before a code would not fit"""
        nonlocal acc, nacc
        entries = 258 + max(codes - 1, 0)
        width = 9 + (entries >= 511) + (entries >= 1023) + (entries >= 2047)
        acc = (acc << width) | code
        nacc += width
        while nacc >= 8:
            nacc -= 8
            out.append((acc >> nacc) & 255)
        acc &= (1 << nacc) - 1

    emit(256)
    for b in bytes(data):
        if w < 0:
            w = b
            continue
        key = (w << 8) | b
        hit = table.get(key)
        if hit is not None:
            w = hit
            continue
        emit(w)
        codes += 1
        table[key] = free
        free += 1
        w = b
        if free == 4094:
            emit(256)
            table, free, codes = {}, 258, 0
    if w >= 0:
        emit(w)
        codes += 1
    emit(257)
    if nacc:
        out.append((acc << (8 - nacc)) & 255)
    return bytes(out)


def packbits_encode(row):
    """one row: runs of three or more equal bytes as repeats, the rest as literals of at most 128"""
    row = bytes(row)
    out = bytearray()
    i, n = 0, len(row)
    lit = bytearray()

    def flush():
        for k in range(0, len(lit), 128):
            piece = lit[k:k + 128]
            out.append(len(piece) - 1)
            out.extend(piece)
        lit.clear()

    while i < n:
        j = i
        while j < n and row[j] == row[i] and j - i < 128:
            j += 1
        if j - i >= 3:
            flush()
            out.append(257 - (j - i))
            out.append(row[i])
        else:
            lit.extend(row[i:j])
        i = j
    flush()
    return bytes(out)


def _segment_bytes(seg, order, predictor):
    """[rows, cols, sps] native samples -> the bytes a writer hands to the compressor"""
    rows, cols, sps = seg.shape
    item = seg.dtype.itemsize
    if predictor == 3:
        be = np.ascontiguousarray(seg.astype(">f4")).view(np.uint8).reshape(rows, cols * sps, 4)
        planes = np.ascontiguousarray(be.transpose(0, 2, 1)).reshape(rows, 4 * cols, sps)
        diff = planes.copy()
        diff[:, 1:] = planes[:, 1:] - planes[:, :-1]  # uint8 arithmetic wraps
        return diff.tobytes()
    u = np.ascontiguousarray(seg).view(f"u{item}")
    if predictor == 2:
        diff = u.copy()
        diff[:, 1:] = u[:, 1:] - u[:, :-1]  # modular in the sample's width
        u = diff
    return (u.byteswap() if order == ">" and item > 1 else u).tobytes()


def _compress(raw, compression, row_bytes, zlib_level=6, cache=None):
    if compression == NONE:
        return raw
    if compression == DEFLATE:
        return zlib.compress(raw, zlib_level)
    if compression == PACKBITS:
        return b"".join(packbits_encode(raw[k:k + row_bytes]) for k in range(0, len(raw), row_bytes))
    if cache is None:
        return lzw_encode(raw)
    key = hashlib.blake2b(raw, digest_size=16).digest()
    if key not in cache:
        cache[key] = lzw_encode(raw)
    return cache[key]


def write_tiff(path, pixels, order="<", tile=None, rows_per_strip=None, planar=1, compression=NONE, predictor=1,
               predictor_tag=None, override=None, zlib_level=6, workers=1, lzw_cache=None):
    """pixels [H, W] or [H, W, C] of uint8 / uint16 / int16 / float32.  tile (rows, cols) or strips of rows_per_strip
    rows (default: one strip); planar 2 writes one plane per sample; order "<" / ">".  predictor_tag writes tag 317
    without differencing (what libtiff does under PackBits and no compression).  override {code: (type, values)}
    replaces or adds tags as they are (for the files a reader must refuse).  For large rasters (tools/tiff_bench.py):
    zlib_level, workers (threads that compress segments) and lzw_cache, a dict that keeps the LZW stream of every
    distinct segment, so that a raster made of equal tiles is encoded once."""
    a = np.asarray(pixels)
    a = a[:, :, None] if a.ndim == 2 else a
    h, w, spp = a.shape
    item = a.dtype.itemsize
    fmt = {"u": 1, "i": 2, "f": 3}[a.dtype.kind]
    planes = [a[:, :, c:c + 1] for c in range(spp)] if planar == 2 and spp > 1 else [a]
    seg_rows, seg_cols = tile if tile else (rows_per_strip or h, w)
    jobs = [(plane, y0, x0) for plane in planes for y0 in range(0, h, seg_rows) for x0 in range(0, w, seg_cols)]

    def encode(job):
        plane, y0, x0 = job
        part = plane[y0:y0 + seg_rows, x0:x0 + seg_cols]
        if tile and part.shape[:2] != (seg_rows, seg_cols):  # a tile is always whole: pad with zeros
            full = np.zeros((seg_rows, seg_cols, part.shape[2]), a.dtype)
            full[:part.shape[0], :part.shape[1]] = part
            part = full
        raw = _segment_bytes(part, order, predictor)
        return _compress(raw, compression, seg_cols * part.shape[2] * item, zlib_level, lzw_cache)

    if workers > 1 and compression == DEFLATE:  # zlib releases the interpreter lock; the Python encoders do not
        with ThreadPoolExecutor(workers) as pool:
            segments = list(pool.map(encode, jobs))
    else:
        segments = [encode(j) for j in jobs]
    offsets, ifd_at = [], 8
    for seg in segments:
        offsets.append(ifd_at)
        ifd_at += len(seg) + (len(seg) & 1)
    if ifd_at >= 1 << 32:
        raise ValueError("classic TIFF: the file would pass 4 GiB")
    extra = bytearray()
    def field(typ, vals):
        code = {3: "H", 4: "I"}[typ]
        raw = struct.pack(f"{order}{len(vals)}{code}", *vals)
        if len(raw) <= 4:
            return raw.ljust(4, b"\0")
        at = len(extra)
        extra.extend(raw + b"\0" * (len(raw) & 1))
        return ("extra", at)

    rgb = spp == 3 and a.dtype == np.uint8
    tags = [(256, 4, [w]), (257, 4, [h]), (258, 3, [8 * item] * spp), (259, 3, [compression]),
            (262, 3, [2 if rgb else 1]), (277, 3, [spp]), (284, 3, [planar if spp > 1 else 1]), (339, 3, [fmt] * spp)]
    if tile:
        tags += [(322, 3, [seg_cols]), (323, 3, [seg_rows]), (324, 4, offsets), (325, 4, [len(s) for s in segments])]
    else:
        tags += [(273, 4, offsets), (278, 4, [seg_rows]), (279, 4, [len(s) for s in segments])]
    if predictor > 1 or predictor_tag:
        tags.append((317, 3, [predictor_tag or predictor]))
    if spp > 1 and not rgb:
        tags.append((338, 3, [0] * (spp - 1)))
    for code, (typ, vals) in (override or {}).items():
        tags = [t for t in tags if t[0] != code] + [(code, typ, list(vals))]
    tags.sort()
    extra_at = ifd_at + 2 + 12 * len(tags) + 4
    entries = b""
    for code, typ, vals in tags:
        f = field(typ, vals)
        if isinstance(f, tuple):
            f = struct.pack(order + "I", extra_at + f[1])
        entries += struct.pack(order + "HHI", code, typ, len(vals)) + f
    with open(path, "wb") as out:
        out.write((b"II" if order == "<" else b"MM") + struct.pack(order + "HI", 42, ifd_at))
        for seg in segments:
            out.write(seg + b"\0" * (len(seg) & 1))
        out.write(struct.pack(order + "H", len(tags)) + entries + struct.pack(order + "I", 0))
        out.write(extra)


def pixels(mode, h=H, w=W):
    rng = np.random.default_rng({"u8": 1, "u16": 2, "rgb": 3, "f32": 4}[mode])
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = 30.0 * np.cos(xx / 5.0) + 2.0 * yy
    if mode == "u8":
        return np.clip(ramp + 100 + rng.integers(0, 5, (h, w)), 0, 255).astype(np.uint8)
    if mode == "u16":
        return (ramp * 200 + 20000 + rng.integers(0, 400, (h, w))).astype(np.uint16)
    if mode == "rgb":
        return np.clip(np.stack([ramp + 90, 180 - ramp, yy * 5.0], axis=2) + rng.integers(0, 7, (h, w, 3)), 0,
                       255).astype(np.uint8)
    return (ramp * 0.21 - 7.25 + rng.random((h, w))).astype(np.float32)


def variants():
    """every layout the writer is used for, as (id, mode, write_tiff keywords)"""
    out = []
    for mode in ("u8", "u16", "rgb", "f32"):
        codecs = [(NONE, 1), (PACKBITS, 1), (LZW, 1), (DEFLATE, 1), (LZW, 2), (DEFLATE, 2)]
        if mode == "f32":
            codecs += [(LZW, 3), (DEFLATE, 3)]
        for order in "<>":
            for layout, kw in (("strips", {"rows_per_strip": ROWS}), ("tiles", {"tile": TILE})):
                for planar in ((1, 2) if mode == "rgb" else (1,)):
                    for compression, predictor in codecs:
                        name = (f"{mode}-{'II' if order == '<' else 'MM'}-{layout}-p{planar}-"
                                f"{ {1: 'none', 5: 'lzw', 8: 'deflate', 32773: 'packbits'}[compression]}-pred{predictor}")
                        out.append((name, mode, dict(kw, order=order, planar=planar, compression=compression,
                                                     predictor=predictor)))
    return out


def pil_reads(name):
    """PIL returns big-endian float32 unswapped: those variants are checked against the writer's input only"""
    return not name.startswith("f32-MM-")


def rewrite_scenes(base, how):
    """Rewrites the scene rasters of loader_cases.write_data_dir's GRSS2013 and AVON directories, and of
    write_grss2018_dir's, in place, pixels unchanged: how = "tiles" (16 x 16 tiles + LZW + Predictor 2) or "strips" (one row per strip, big-endian)."""
    import os

    from hypelcnn_amd.common.tiff_io import imread
    kw = {"tiles": dict(tile=TILE, compression=LZW, predictor=2), "strips": dict(rows_per_strip=1, order=">")}[how]
    for rel in ("2013_DFTC/2013_IEEE_GRSS_DF_Contest_CASI.tif", "2013_DFTC/2013_IEEE_GRSS_DF_Contest_LiDAR.tif",
                "AVON/0920-1857.georef_cropped.tif", "AVON/0920-1857.georef_cropped_shcorrected.tif",
                "2018/20170218_UH_CASI_S4_NAD83.tiff", "2018/UH17c_GEF051.tif"):
        path = os.path.join(base, rel)
        if not os.path.exists(path):
            continue
        write_tiff(path, imread(path), **kw)
    return base


def grss2018_pixels():
    """casi [12, 16, 8 + 2] uint16 (the loader drops the last two bands) at half the resolution of lidar [24, 32]
    float32, some of whose heights are above the 300 the loader zeroes"""
    rng = np.random.default_rng(2018)
    casi = rng.integers(200, 9000, (12, 16, 10)).astype(np.uint16)
    lidar = (rng.random((24, 32)) * 60 + 2).astype(np.float32)
    lidar[rng.random((24, 32)) < 0.05] = 977.5
    return casi, lidar


def write_grss2018_dir(base):
    """<base>/2018 with the two scene rasters of GRSS2018DataLoader, as imwrite writes them"""
    import os

    from hypelcnn_amd.common.tiff_io import imwrite
    d = os.path.join(base, "2018")
    os.makedirs(d, exist_ok=True)
    casi, lidar = grss2018_pixels()
    imwrite(os.path.join(d, "20170218_UH_CASI_S4_NAD83.tiff"), casi)
    imwrite(os.path.join(d, "UH17c_GEF051.tif"), lidar)
    return base
