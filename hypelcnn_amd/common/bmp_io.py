"""Minimal BMP reader for the AVON target masks (the reference reads them with imageio.v2.imread,
loader/AVONDataLoader.py:82-88; imageio is not a dependency of this project).

Uncompressed (BI_RGB) files with a BITMAPINFOHEADER or one of its longer successors, stored bottom-up (positive
height) or top-down (negative height): 1 bit per pixel -> bool [H, W] (palette entry 0 / 1, as imageio hands a
two-colour black-and-white bitmap over), 8 bits -> uint8 [H, W] when the palette is a gray ramp, else the
palette's RGB as uint8 [H, W, 3], 24 bits -> uint8 [H, W, 3] in RGB order.  Anything else raises ValueError."""
import struct

import numpy


def imread(path):
    raw = open(path, "rb").read()
    if len(raw) < 54 or raw[:2] != b"BM":
        raise ValueError("bmp_io.imread: not a BMP file")
    data_off = struct.unpack_from("<I", raw, 10)[0]
    header = struct.unpack_from("<I", raw, 14)[0]
    if header < 40:
        raise ValueError("bmp_io.imread: BITMAPCOREHEADER files are not supported")
    w, h, planes, bits, compression = struct.unpack_from("<iiHHI", raw, 18)
    colours = struct.unpack_from("<I", raw, 46)[0]
    if compression != 0 or planes != 1 or w <= 0 or h == 0:
        raise ValueError("bmp_io.imread: only uncompressed single-plane bitmaps are supported")
    if bits not in (1, 8, 24):
        raise ValueError(f"bmp_io.imread: {bits} bits per pixel not supported (1, 8 or 24)")
    rows, top_down = abs(h), h < 0
    stride = ((w * bits + 31) // 32) * 4
    if data_off + stride * rows > len(raw):
        raise ValueError("bmp_io.imread: truncated pixel data")
    lines = numpy.frombuffer(raw, numpy.uint8, stride * rows, data_off).reshape(rows, stride)
    if not top_down:
        lines = lines[::-1]
    if bits == 24:
        return numpy.ascontiguousarray(lines[:, :w * 3].reshape(rows, w, 3)[:, :, ::-1])
    n_pal = colours if colours else (1 << bits)
    if 14 + header + n_pal * 4 > data_off:
        raise ValueError("bmp_io.imread: a palette bitmap without room for its palette is not supported")
    palette = numpy.frombuffer(raw, numpy.uint8, n_pal * 4, 14 + header).reshape(n_pal, 4)[:, 2::-1]
    if bits == 1:
        index = numpy.unpackbits(lines, axis=1)[:, :w]
        if n_pal < 2 or int(palette[0].sum()) <= int(palette[1].sum()):
            return index.astype(bool)
        return numpy.logical_not(index)  # inverted palette: entry 0 is the white one
    index = numpy.ascontiguousarray(lines[:, :w])
    if (palette[:, 0] == palette[:, 1]).all() and (palette[:, 0] == palette[:, 2]).all():
        lut = numpy.zeros(256, numpy.uint8)
        lut[:n_pal] = palette[:, 0]
        return lut[index]
    lut = numpy.zeros((256, 3), numpy.uint8)
    lut[:n_pal] = palette
    return lut[index]
