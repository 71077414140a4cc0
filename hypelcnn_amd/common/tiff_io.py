"""TIFF for the rasters: a minimal baseline writer for the results (the reference uses tifffile.imwrite,
classify/infer_for_classification.py:67-68, gan/gan_infer_image_for_shadow.py:93; tifffile is not available in this
image) and a reader for what GDAL, ENVI and libtiff tools write (the reference's tifffile.imread reads anything).

imwrite: uncompressed, little-endian, one strip: uint8 grayscale [H,W] or RGB [H,W,3], and multi-band [H,W,C] rasters
of float32 / uint16 / int16 / uint8 stored chunky (planarconfig="contig": the C samples of a pixel next to each other).

read_layout / imread / read_raster: the first image of a classic TIFF in either byte order, in strips or tiles, chunky
or planar, uncompressed or PackBits / LZW / Deflate with Predictor 1, 2 or 3, of the four dtypes above.  imread decodes
on the host; read_raster(path, backend) leaves the scene on the device (csrc/tiff.hip): segment decoding, predictor,
byte swap, de-tiling and plane interleave run in front of the scene preparation, where the file's bytes already are."""
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy

# dtype -> (BitsPerSample, SampleFormat: 1 unsigned integer, 2 signed integer, 3 IEEE float)
_FORMATS = {numpy.dtype(numpy.uint8): (8, 1), numpy.dtype(numpy.uint16): (16, 1), numpy.dtype(numpy.int16): (16, 2),
            numpy.dtype(numpy.float32): (32, 3)}


def imwrite(path, image):
    img = numpy.ascontiguousarray(image)
    if img.dtype not in _FORMATS or img.ndim not in (2, 3):
        raise ValueError("imwrite: [H,W] or [H,W,C] of uint8, uint16, int16 or float32 expected")
    if img.dtype == numpy.uint8 and (img.ndim == 2 or img.shape[2] == 3):
        _write_gray_rgb8(path, img)
    else:
        _write_chunky(path, img if img.ndim == 3 else img[:, :, None])


def _write_gray_rgb8(path, img):
    h, w = img.shape[:2]
    spp = 1 if img.ndim == 2 else 3
    data = img.tobytes()
    entries = []

    def tag(code, typ, count, value):
        entries.append(struct.pack("<HHII", code, typ, count, value))

    n_tags = 10 if spp == 1 else 10
    ifd_off = 8 + len(data) + (len(data) & 1)
    extra_off = ifd_off + 2 + n_tags * 12 + 4
    tag(256, 4, 1, w)                      # ImageWidth
    tag(257, 4, 1, h)                      # ImageLength
    if spp == 1:
        tag(258, 3, 1, 8)                  # BitsPerSample
    else:
        tag(258, 3, 3, extra_off)          # -> three shorts after the IFD
    tag(259, 3, 1, 1)                      # no compression
    tag(262, 3, 1, 1 if spp == 1 else 2)   # BlackIsZero / RGB
    tag(273, 4, 1, 8)                      # StripOffsets
    tag(277, 3, 1, spp)                    # SamplesPerPixel
    tag(278, 4, 1, h)                      # RowsPerStrip
    tag(279, 4, 1, len(data))              # StripByteCounts
    tag(284, 3, 1, 1)                      # PlanarConfiguration: chunky
    with open(path, "wb") as f:
        f.write(b"II*\x00" + struct.pack("<I", ifd_off))
        f.write(data)
        if len(data) & 1:
            f.write(b"\x00")
        f.write(struct.pack("<H", len(entries)) + b"".join(entries) + struct.pack("<I", 0))
        if spp == 3:
            f.write(struct.pack("<HHH", 8, 8, 8))


def _write_chunky(path, img):
    """[H,W,C] minisblack with C - 1 unspecified extra samples (what tifffile writes for planarconfig="contig")."""
    h, w, spp = img.shape
    bits, fmt = _FORMATS[img.dtype]
    data = img.astype(img.dtype.newbyteorder("<"), copy=False).tobytes()
    n_tags = 11 + (spp > 1)
    ifd_off = 8 + len(data) + (len(data) & 1)
    extra_off = ifd_off + 2 + n_tags * 12 + 4
    extra = b""

    def per_sample(value):
        """SHORT x spp: inline when it fits the 4-byte value field, else after the IFD"""
        nonlocal extra
        if spp <= 2:
            return struct.unpack("<I", struct.pack("<" + "H" * spp, *([value] * spp)).ljust(4, b"\x00"))[0]
        off = extra_off + len(extra)
        extra += struct.pack("<" + "H" * spp, *([value] * spp))
        return off

    entries = [(256, 4, 1, w), (257, 4, 1, h), (258, 3, spp, per_sample(bits)), (259, 3, 1, 1), (262, 3, 1, 1),
               (273, 4, 1, 8), (277, 3, 1, spp), (278, 4, 1, h), (279, 4, 1, len(data)), (284, 3, 1, 1)]
    if spp > 1:
        if spp - 1 <= 2:
            entries.append((338, 3, spp - 1, 0))  # ExtraSamples: unspecified (zeros, inline)
        else:
            entries.append((338, 3, spp - 1, extra_off + len(extra)))
            extra += b"\x00\x00" * (spp - 1)
    entries.append((339, 3, spp, per_sample(fmt)))  # SampleFormat
    entries.sort()
    assert len(entries) == n_tags
    with open(path, "wb") as f:
        f.write(b"II*\x00" + struct.pack("<I", ifd_off))
        f.write(data)
        if len(data) & 1:
            f.write(b"\x00")
        f.write(struct.pack("<H", n_tags) + b"".join(struct.pack("<HHII", *e) for e in entries) + struct.pack("<I", 0))
        f.write(extra)




# ---------------------------------------------------------------------------------------------------- reading
COMPRESSION_NONE, COMPRESSION_LZW, COMPRESSION_DEFLATE, COMPRESSION_PACKBITS = 1, 5, 8, 32773
_DEFLATE_CODES = (8, 32946)
_REFUSED_COMPRESSIONS = {2: "CCITT RLE", 3: "CCITT T.4", 4: "CCITT T.6", 6: "old-style JPEG", 7: "JPEG",
                         34712: "JPEG 2000", 34925: "LZMA", 50000: "ZSTD", 50001: "WebP", 50002: "JPEG XL"}
_TYPE_SIZES = {1: (1, "B"), 3: (2, "H"), 4: (4, "I")}  # BYTE, SHORT, LONG: what the tags read here may be stored as
_DTYPES = {(8, 1): numpy.uint8, (16, 1): numpy.uint16, (16, 2): numpy.int16, (32, 3): numpy.float32}
POOL_WORKERS = 16  # segment-level host work (zlib); a constant, not the machine's core count
# status of a segment after hypel_tiff_unpack (include/hypel.h HYPEL_TIFF_*) and of the host decoders' refusals
UNPACK_ERRORS = {1: "a code above the next free one", 2: "the first code is not a literal",
                 3: "the stream ends before the segment is complete", 4: "the segment's range lies outside its buffer"}


class TiffLayout:
    """How the first image of a TIFF file is laid out: everything the readers need, nothing decoded.

    byteorder "II" / "MM"; width, height, spp, dtype; compression (1 none, 5 LZW, 8 Deflate -- 32946 is reported
    as 8 -- 32773 PackBits); predictor as it APPLIES (1, 2, 3: the tag counts only under LZW and Deflate); planar
    (1 chunky, 2 one plane per sample); tiled; seg_rows x seg_cols pixels per segment (a strip is `width` columns);
    segs_across x segs_down segments per plane; offsets / counts per segment, plane-major; file_size."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def item(self):
        return numpy.dtype(self.dtype).itemsize

    @property
    def planes(self):
        return self.spp if self.planar == 2 else 1

    @property
    def sps(self):
        """samples of a pixel inside one segment"""
        return 1 if self.planar == 2 else self.spp

    @property
    def row_bytes(self):
        return self.seg_cols * self.sps * self.item

    @property
    def n_segments(self):
        return self.planes * self.segs_across * self.segs_down

    def segment_rows(self, i):
        """rows segment i stores: a tile is always whole, the last strip holds what is left of the image"""
        if self.tiled:
            return self.seg_rows
        sy = (i % (self.segs_across * self.segs_down)) // self.segs_across
        return min(self.seg_rows, self.height - sy * self.seg_rows)

    def segment_bytes(self, i):
        return self.segment_rows(i) * self.row_bytes

    @property
    def shape(self):
        return (self.height, self.width) if self.spp == 1 else (self.height, self.width, self.spp)

    @property
    def in_place(self):
        """the file's samples are the raster already: little-endian, uncompressed (a predictor tag is ignored then),
        chunky, strips one behind the other in ascending order"""
        if self.byteorder != "II" or self.compression != COMPRESSION_NONE or self.planes != 1 or self.tiled:
            return False
        at = self.offsets[0]
        for i, off in enumerate(self.offsets):
            if off != at:
                return False
            at += self.segment_bytes(i)
        return True


def _tag_values(buf, bo, typ, count, field_at, name):
    if typ not in _TYPE_SIZES:
        raise ValueError(f"tiff_io: tag {name} has type {typ}; BYTE, SHORT or LONG expected")
    size, fmt = _TYPE_SIZES[typ]
    at = field_at if size * count <= 4 else struct.unpack_from(bo + "I", buf, field_at)[0]
    if at + size * count > len(buf):
        raise ValueError(f"tiff_io: the values of tag {name} reach past the end of the file")
    return list(struct.unpack_from(f"{bo}{count}{fmt}", buf, at))


def _parse(buf):
    if len(buf) < 8 or bytes(buf[:2]) not in (b"II", b"MM"):
        raise ValueError("tiff_io: not a TIFF file")
    order = bytes(buf[:2]).decode()
    bo = "<" if order == "II" else ">"
    magic = struct.unpack_from(bo + "H", buf, 2)[0]
    if magic == 43:
        raise ValueError("tiff_io: BigTIFF is not supported")
    if magic != 42:
        raise ValueError("tiff_io: not a TIFF file")
    ifd = struct.unpack_from(bo + "I", buf, 4)[0]
    if ifd + 2 > len(buf):
        raise ValueError("tiff_io: the first IFD lies past the end of the file")
    n = struct.unpack_from(bo + "H", buf, ifd)[0]
    if ifd + 2 + 12 * n > len(buf):
        raise ValueError("tiff_io: the first IFD reaches past the end of the file")
    tags = {}
    for i in range(n):
        at = ifd + 2 + 12 * i
        code, typ, count = struct.unpack_from(bo + "HHI", buf, at)
        tags[code] = (typ, count, at + 8)

    def values(code, name, default=None):
        if code not in tags:
            if default is None:
                raise ValueError(f"tiff_io: tag {name} is missing")
            return default
        return _tag_values(buf, bo, *tags[code], name)

    w, h = values(256, "ImageWidth")[0], values(257, "ImageLength")[0]
    spp = values(277, "SamplesPerPixel", [1])[0]
    if w < 1 or h < 1 or spp < 1:
        raise ValueError("tiff_io: empty image")
    compression = values(259, "Compression", [1])[0]
    if compression in _DEFLATE_CODES:
        compression = COMPRESSION_DEFLATE
    if compression not in (COMPRESSION_NONE, COMPRESSION_LZW, COMPRESSION_DEFLATE, COMPRESSION_PACKBITS):
        raise ValueError(f"tiff_io: {_REFUSED_COMPRESSIONS.get(compression, f'compression {compression}')} "
                         "is not supported (none, LZW, Deflate and PackBits are)")
    if values(266, "FillOrder", [1])[0] != 1:
        raise ValueError("tiff_io: FillOrder 2 is not supported")
    if values(274, "Orientation", [1])[0] != 1:
        raise ValueError("tiff_io: only Orientation 1 (top left) is supported")
    bits = set(values(258, "BitsPerSample", [1]))
    fmt = set(values(339, "SampleFormat", [1]))
    if len(bits) != 1 or len(fmt) != 1:
        raise ValueError("tiff_io: mixed sample formats are not supported")
    bits, fmt = bits.pop(), fmt.pop()
    fmt = 1 if fmt == 4 else fmt  # "undefined" is read as unsigned, as libtiff does
    if bits % 8:
        raise ValueError(f"tiff_io: sub-byte samples ({bits} bits) are not supported")
    if bits == 32 and fmt in (1, 2):
        raise ValueError("tiff_io: 32-bit integers are not supported")
    if bits == 64:
        raise ValueError("tiff_io: float64 and 64-bit samples are not supported")
    if (bits, fmt) not in _DTYPES:
        raise ValueError(f"tiff_io: unsupported sample format ({bits} bits, SampleFormat {fmt})")
    dtype = numpy.dtype(_DTYPES[(bits, fmt)])
    planar = values(284, "PlanarConfiguration", [1])[0]
    if planar not in (1, 2):
        raise ValueError(f"tiff_io: PlanarConfiguration {planar} is not defined")
    if spp == 1:
        planar = 1
    predictor = values(317, "Predictor", [1])[0]
    if predictor not in (1, 2, 3):
        raise ValueError(f"tiff_io: Predictor {predictor} is not defined")
    if compression not in (COMPRESSION_LZW, COMPRESSION_DEFLATE):
        predictor = 1  # libtiff's raw and PackBits codecs never install the predictor: the tag is ignored
    if predictor == 3 and dtype != numpy.float32:
        raise ValueError("tiff_io: Predictor 3 (floating point) on non-float samples")
    tiled = 322 in tags or 324 in tags
    if tiled:
        seg_cols, seg_rows = values(322, "TileWidth")[0], values(323, "TileLength")[0]
        offsets, counts = values(324, "TileOffsets"), values(325, "TileByteCounts")
    else:
        seg_cols, seg_rows = w, min(values(278, "RowsPerStrip", [h])[0], h)
        offsets, counts = values(273, "StripOffsets"), values(279, "StripByteCounts")
    if seg_cols < 1 or seg_rows < 1:
        raise ValueError("tiff_io: empty segments")
    lay = TiffLayout(byteorder=order, width=w, height=h, spp=spp, dtype=dtype, compression=compression,
                     predictor=predictor, planar=planar, tiled=tiled, seg_rows=seg_rows, seg_cols=seg_cols,
                     segs_across=-(-w // seg_cols), segs_down=-(-h // seg_rows), offsets=offsets, counts=counts,
                     file_size=len(buf))
    if len(offsets) != len(counts):
        raise ValueError(f"tiff_io: {len(offsets)} segment offsets but {len(counts)} byte counts")
    if len(offsets) != lay.n_segments:
        raise ValueError(f"tiff_io: {len(offsets)} segments in the file, the geometry needs {lay.n_segments}")
    for i, (off, cnt) in enumerate(zip(offsets, counts)):
        if off + cnt > len(buf):
            raise ValueError(f"tiff_io: segment {i} reaches past the end of the file")
        if compression == COMPRESSION_NONE and cnt < lay.segment_bytes(i):
            raise ValueError(f"tiff_io: segment {i} holds {cnt} bytes, the geometry needs {lay.segment_bytes(i)}")
    if compression == COMPRESSION_LZW:
        for off, cnt in zip(offsets, counts):
            if cnt >= 2 and buf[off] == 0 and buf[off + 1] & 1:  # libtiff's test
                raise ValueError("tiff_io: old-style LZW (bit-reversed codes) is not supported")
    return lay


def read_layout(path):
    """TiffLayout of the first IFD of `path`.  GeoTIFF and other unknown tags are ignored; what cannot be read is
    refused by name with ValueError (BigTIFF, any compression but none / LZW / Deflate / PackBits, old-style LZW,
    FillOrder 2, Orientation != 1, sub-byte, mixed, 32-bit integer and float64 samples, Predictor 3 on non-float
    data, segment tables that do not match the geometry or reach past the end of the file)."""
    if os.path.getsize(path) < 8:
        raise ValueError("tiff_io: not a TIFF file")
    return _parse(numpy.memmap(path, numpy.uint8, "r"))


def lzw_decode(data, need):
    """TIFF LZW (MSB-first codes, Clear 256, EOI 257, first free 258, 9 bits growing at 511 / 1023 / 2047 -- "early
    change") -> `need` bytes.  Plain Python: fine for a label raster, slow for a scene."""
    data = bytes(data)
    out = bytearray()
    table = [bytes([i]) for i in range(256)] + [b"", b""]
    bitpos, nbits, width, prev = 0, len(data) * 8, 9, None
    while len(out) < need:
        if bitpos + width > nbits:
            raise ValueError(UNPACK_ERRORS[3])
        at = bitpos >> 3
        code = (int.from_bytes(data[at:at + 3].ljust(3, b"\0"), "big") >> (24 - (bitpos & 7) - width)) & ((1 << width) - 1)
        bitpos += width
        if code == 257:
            break
        if code == 256:
            del table[258:]
            width, prev = 9, None
            continue
        if prev is None:
            if code > 255:
                raise ValueError(UNPACK_ERRORS[2])
            s = table[code]
        else:
            if code < len(table):
                s = table[code]
                new = prev + s[:1]
            elif code == len(table):
                s = new = prev + prev[:1]
            else:
                raise ValueError(UNPACK_ERRORS[1])
            if len(table) < 4096:
                table.append(new)
        out += s
        prev = s
        nxt = len(table)
        width = 9 + (nxt >= 511) + (nxt >= 1023) + (nxt >= 2047)
    if len(out) < need:
        raise ValueError(UNPACK_ERRORS[3])
    return bytes(out[:need])


def packbits_decode(data, need):
    """PackBits: header n in 0..127 copies n + 1 literals, -127..-1 repeats the next byte 1 - n times, -128 is a
    no-op; the last run is clipped at `need`.  Plain Python."""
    data = bytes(data)
    out = bytearray()
    at = 0
    while len(out) < need:
        if at >= len(data):
            raise ValueError(UNPACK_ERRORS[3])
        n = data[at]
        at += 1
        if n < 128:
            lit = data[at:at + n + 1]
            out += lit
            at += n + 1
            if len(lit) < n + 1 and len(out) < need:
                raise ValueError(UNPACK_ERRORS[3])
        elif n > 128:
            if at >= len(data):
                raise ValueError(UNPACK_ERRORS[3])
            out += data[at:at + 1] * (257 - n)
            at += 1
    return bytes(out[:need])


def _decode_segment(buf, lay, i):
    off, cnt, need = lay.offsets[i], lay.counts[i], lay.segment_bytes(i)
    try:
        if lay.compression == COMPRESSION_NONE:
            return bytes(buf[off:off + need])
        data = bytes(buf[off:off + cnt])
        if lay.compression == COMPRESSION_DEFLATE:
            out = zlib.decompressobj().decompress(data, need)
            if len(out) < need:
                raise ValueError(UNPACK_ERRORS[3])
            return out
        if lay.compression == COMPRESSION_LZW:
            return lzw_decode(data, need)
        return packbits_decode(data, need)
    except (ValueError, zlib.error) as e:
        raise ValueError(f"tiff_io: segment {i}: {e}") from None


def _decode_all(buf, lay):
    idx = range(lay.n_segments)
    if lay.compression == COMPRESSION_DEFLATE and lay.n_segments > 1:
        with ThreadPoolExecutor(min(POOL_WORKERS, lay.n_segments)) as pool:  # zlib releases the GIL
            return list(pool.map(lambda i: _decode_segment(buf, lay, i), idx))
    return [_decode_segment(buf, lay, i) for i in idx]


def _segment_samples(lay, seg, rows):
    """decoded bytes of a segment -> [rows, seg_cols, sps] in the raster's dtype, native order, predictor undone"""
    n, item = lay.seg_cols * lay.sps, lay.item
    raw = numpy.frombuffer(seg, numpy.uint8, rows * n * item)
    if lay.predictor == 3:
        acc = numpy.cumsum(raw.reshape(rows, lay.seg_cols * item, lay.sps), axis=1, dtype=numpy.uint8)
        planes = acc.reshape(rows, item, n)  # byte planes of the row, most significant first
        return numpy.ascontiguousarray(planes.transpose(0, 2, 1)).view(">f4").astype(numpy.float32).reshape(
            rows, lay.seg_cols, lay.sps)
    uint = numpy.dtype(f"u{item}")
    v = raw.view(uint.newbyteorder("<" if lay.byteorder == "II" else ">")).astype(uint).reshape(rows, lay.seg_cols, lay.sps)
    if lay.predictor == 2:
        v = numpy.cumsum(v, axis=1, dtype=uint)  # modular in the sample's width; float32 as 32-bit integers
    return v.view(lay.dtype)


def _assemble_host(lay, segments):
    out = numpy.empty((lay.height, lay.width, lay.spp), lay.dtype)
    per_plane = lay.segs_across * lay.segs_down
    for i, seg in enumerate(segments):
        plane, rest = divmod(i, per_plane)
        sy, sx = divmod(rest, lay.segs_across)
        rows = lay.segment_rows(i)
        tile = _segment_samples(lay, seg, rows)
        y0, x0 = sy * lay.seg_rows, sx * lay.seg_cols
        hh, ww = min(rows, lay.height - y0), min(lay.seg_cols, lay.width - x0)
        if lay.planar == 2:
            out[y0:y0 + hh, x0:x0 + ww, plane] = tile[:hh, :ww, 0]
        else:
            out[y0:y0 + hh, x0:x0 + ww, :] = tile[:hh, :ww, :]
    return out


def imread(path):
    """The first image of a TIFF file as [H, W] (one sample per pixel) or [H, W, C] of uint8, uint16, int16 or
    float32, decoded on the host: strips or tiles, chunky or planar, either byte order, no compression, PackBits,
    LZW or Deflate, Predictor 1, 2 or 3 (read_layout lists what is refused).  Deflate goes through zlib; LZW and
    PackBits through plain Python decoders -- slow for a whole scene, fine for the label rasters and shadow maps
    this is used for; scenes go through read_raster, which decodes those two on the device."""
    buf = numpy.fromfile(path, numpy.uint8)
    lay = _parse(buf)
    if lay.in_place:
        img = numpy.frombuffer(buf, lay.dtype.newbyteorder("<"), lay.height * lay.width * lay.spp, lay.offsets[0])
        return img.astype(lay.dtype).reshape(lay.shape)
    return _assemble_host(lay, _decode_all(buf, lay)).reshape(lay.shape)


# ---------------------------------------------------------------------------------------------------- device path
class DeviceRaster:
    """A raster in device memory: a flat byte tensor, the byte offset of its first sample, dtype, shape and element
    strides.  Supports what the loaders do to a scene -- basic slicing on any axis, numpy.newaxis, swapaxes /
    transpose -- as views without a launch; device_scene reads it through its strides.  download() brings it back."""

    def __init__(self, data, byte_offset, dtype, shape, strides=None):
        self.bytes = data
        self.dtype = numpy.dtype(dtype)
        self.shape = tuple(int(n) for n in shape)
        if strides is None:
            strides, step = [], 1
            for n in reversed(self.shape):
                strides.insert(0, step)
                step *= n
        self.strides = tuple(int(s) for s in strides)
        self.byte_offset = int(byte_offset)

    @property
    def ndim(self):
        return len(self.shape)

    def __getitem__(self, key):
        key = key if isinstance(key, tuple) else (key,)
        if sum(k is Ellipsis for k in key) > 1:
            raise IndexError("an index can only have a single ellipsis")
        n_real = sum(k is not None and k is not Ellipsis for k in key)
        if n_real > self.ndim:
            raise IndexError("too many indices for a DeviceRaster")
        if Ellipsis in key:
            at = key.index(Ellipsis)
            key = key[:at] + (slice(None),) * (self.ndim - n_real) + key[at + 1:]
        else:
            key = key + (slice(None),) * (self.ndim - n_real)
        shape, strides, offset, axis = [], [], 0, 0
        for k in key:
            if k is None:
                shape.append(1)
                strides.append(0)
                continue
            n, s = self.shape[axis], self.strides[axis]
            axis += 1
            if isinstance(k, slice):
                start, stop, step = k.indices(n)
                if step < 1:
                    raise ValueError("DeviceRaster: slices with a positive step only")
                offset += start * s
                shape.append(max(0, -(-(stop - start) // step)))
                strides.append(s * step)
            else:
                i = int(k)
                if not -n <= i < n:
                    raise IndexError(f"index {i} is out of bounds for an axis of size {n}")
                offset += (i % n) * s
        return DeviceRaster(self.bytes, self.byte_offset + offset * self.dtype.itemsize, self.dtype, shape, strides)

    def transpose(self, *axes):
        axes = axes[0] if len(axes) == 1 and not isinstance(axes[0], int) else axes
        axes = tuple(range(self.ndim))[::-1] if not axes else tuple(int(a) % self.ndim for a in axes)
        if sorted(axes) != list(range(self.ndim)):
            raise ValueError("axes don't match the raster")
        return DeviceRaster(self.bytes, self.byte_offset, self.dtype, [self.shape[a] for a in axes],
                            [self.strides[a] for a in axes])

    def swapaxes(self, a, b):
        axes = list(range(self.ndim))
        axes[a], axes[b] = axes[b], axes[a]
        return self.transpose(axes)

    def astype(self, dtype, copy=True):
        if numpy.dtype(dtype) != self.dtype:
            raise ValueError(f"DeviceRaster: no conversion on the device ({self.dtype} -> {numpy.dtype(dtype)})")
        return self

    def download(self):
        """the raster as a host array (a copy of the tensor's bytes it spans)"""
        if 0 in self.shape:
            return numpy.empty(self.shape, self.dtype)
        item = self.dtype.itemsize
        span = (sum((n - 1) * s for n, s in zip(self.shape, self.strides)) + 1) * item
        host = self.bytes[self.byte_offset:self.byte_offset + span].cpu().numpy().copy()
        return numpy.lib.stride_tricks.as_strided(host.view(self.dtype), self.shape, [s * item for s in self.strides])

    def __array__(self, dtype=None, copy=None):
        a = self.download()
        return a if dtype is None else a.astype(dtype)


def segment_table(lay, dst_align=16):
    """hypel_tiff_seg_t records of a layout (backend.TIFF_SEG_DTYPE): where each segment lies in the file and where
    its decoded bytes go in a buffer of the returned size (segments one behind the other, aligned)."""
    from hypelcnn_amd.backend import TIFF_SEG_DTYPE
    table = numpy.zeros(lay.n_segments, TIFF_SEG_DTYPE)
    at = 0
    for i in range(lay.n_segments):
        need = lay.segment_bytes(i)
        table[i] = (lay.offsets[i], need if lay.compression == COMPRESSION_NONE else lay.counts[i], at, need)
        at += -(-need // dst_align) * dst_align
    return table, at


def check_segment_table(table, src_bytes, dst_bytes):
    """What the kernels rely on and cannot check as a whole: every src range inside the source buffer, the dst ranges
    inside the decoded buffer and disjoint."""
    t = numpy.asarray(table)
    if t.size == 0:
        raise ValueError("tiff_io: empty segment table")
    if (t["src_off"] < 0).any() or (t["src_len"] < 0).any() or (t["src_off"] + t["src_len"] > src_bytes).any():
        bad = int(numpy.argmax((t["src_off"] < 0) | (t["src_len"] < 0) | (t["src_off"] + t["src_len"] > src_bytes)))
        raise ValueError(f"tiff_io: segment {bad} names a source range outside the file")
    if (t["dst_off"] < 0).any() or (t["dst_len"] < 0).any() or (t["dst_off"] + t["dst_len"] > dst_bytes).any():
        raise ValueError("tiff_io: a segment's decoded range lies outside the buffer")
    order = numpy.argsort(t["dst_off"], kind="stable")
    ends = (t["dst_off"] + t["dst_len"])[order]
    if (ends[:-1] > t["dst_off"][order][1:]).any():
        raise ValueError("tiff_io: decoded ranges of two segments overlap")


def raise_for_status(status, what="tiff_io"):
    bad = numpy.flatnonzero(numpy.asarray(status))
    if bad.size:
        i = int(bad[0])
        code = int(numpy.asarray(status)[i])
        raise ValueError(f"{what}: segment {i}: {UNPACK_ERRORS.get(code, f'status {code}')}")


def read_raster(path, backend):
    """The first image of `path`: imread's array when `backend` is None, else a DeviceRaster.

    On the device the file is uploaded once (for Deflate: the segments inflated on the host with zlib instead),
    hypel_tiff_unpack decodes LZW / PackBits segments, hypel_tiff_assemble undoes predictor, byte order, tiling and
    plane order.  A file that is a raster already (TiffLayout.in_place) is uploaded from its offset on and used as it
    is, without a launch."""
    if backend is None:
        return imread(path)
    import torch
    from hypelcnn_amd.backend import Ref
    buf = numpy.fromfile(path, numpy.uint8)
    lay = _parse(buf)
    if lay.in_place:  # the samples alone are uploaded: the raster starts an allocation, aligned wherever the file had it
        at, size = lay.offsets[0], lay.height * lay.width * lay.spp * lay.item
        return DeviceRaster(backend.upload(buf[at:at + size]), 0, lay.dtype, lay.shape)
    table, dst_bytes = segment_table(lay)
    check_segment_table(table, len(buf), dst_bytes)
    from_decoded = lay.compression != COMPRESSION_NONE
    if lay.compression == COMPRESSION_DEFLATE:
        host = numpy.zeros(dst_bytes, numpy.uint8)
        for rec, seg in zip(table, _decode_all(buf, lay)):
            host[rec["dst_off"]:rec["dst_off"] + rec["dst_len"]] = numpy.frombuffer(seg, numpy.uint8)
        src = backend.upload(host)
    else:
        src = backend.upload(buf)
    table_dev = backend.upload(table)
    if lay.compression in (COMPRESSION_LZW, COMPRESSION_PACKBITS):
        decoded = backend.empty(dst_bytes, torch.uint8)
        status = backend.zeros(lay.n_segments, torch.int32)
        backend.call("tiff_unpack", Ref(src), len(buf), Ref(table_dev), lay.n_segments, lay.compression,
                     Ref(decoded), dst_bytes, Ref(status))
        raise_for_status(status.cpu().numpy(), f"tiff_io: {path}")
        src = decoded
    out = backend.empty(lay.height * lay.width * lay.spp * lay.item, torch.uint8)
    backend.call("tiff_assemble", Ref(src), int(src.numel()), Ref(table_dev), lay.n_segments, int(from_decoded),
                 lay.height, lay.width, lay.spp, lay.item, lay.seg_rows, lay.seg_cols, lay.segs_across, lay.planes,
                 lay.predictor, int(lay.byteorder == "MM"), Ref(out))
    backend.synchronize()  # the operands above are released when this returns
    return DeviceRaster(out, 0, lay.dtype, lay.shape)
