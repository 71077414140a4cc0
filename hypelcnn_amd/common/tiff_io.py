"""Minimal baseline-TIFF writer for the result rasters (the reference uses tifffile.imwrite,
classify/infer_for_classification.py:67-68, gan/gan_infer_image_for_shadow.py:93; tifffile is not available in this
image).

Uncompressed, little-endian, one strip: uint8 grayscale [H,W] or RGB [H,W,3], and multi-band [H,W,C] rasters of
float32 / uint16 / int16 / uint8 stored chunky (planarconfig="contig": the C samples of a pixel next to each other)."""
import struct

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


def _shorts(raw, tag, n):
    typ, count, value = tag
    if count * 2 <= 4:
        return list(struct.unpack_from("<" + "H" * count, struct.pack("<I", value)))
    return list(struct.unpack_from("<" + "H" * count, raw, value))


def imread(path):
    """Reads back what imwrite wrote (and any other uncompressed, single-strip, chunky little-endian TIFF of the
    dtypes imwrite writes)."""
    raw = open(path, "rb").read()
    if raw[:4] != b"II*\x00":
        raise ValueError("imread: little-endian baseline TIFF expected")
    ifd = struct.unpack_from("<I", raw, 4)[0]
    n = struct.unpack_from("<H", raw, ifd)[0]
    tags = {}
    for i in range(n):
        code, typ, count, value = struct.unpack_from("<HHII", raw, ifd + 2 + 12 * i)
        tags[code] = (typ, count, value)
    if tags.get(259, (0, 0, 1))[2] != 1:
        raise ValueError("imread: compressed TIFF not supported")
    w, h, spp = tags[256][2], tags[257][2], tags.get(277, (0, 0, 1))[2]
    off, cnt = tags[273][2], tags[279][2]
    bits = set(_shorts(raw, tags[258], spp)) if 258 in tags else {8}
    fmt = set(_shorts(raw, tags[339], spp)) if 339 in tags else {1}
    if len(bits) != 1 or len(fmt) != 1:
        raise ValueError("imread: mixed sample formats not supported")
    dtype = {(8, 1): numpy.uint8, (16, 1): numpy.uint16, (16, 2): numpy.int16, (32, 3): numpy.float32}.get(
        (bits.pop(), fmt.pop()))
    if dtype is None:
        raise ValueError("imread: unsupported sample format")
    img = numpy.frombuffer(raw, numpy.dtype(dtype).newbyteorder("<"), cnt // numpy.dtype(dtype).itemsize, off)
    img = img.astype(dtype)
    return img.reshape(h, w) if spp == 1 else img.reshape(h, w, spp)
