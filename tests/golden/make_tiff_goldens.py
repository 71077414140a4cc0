#!/usr/bin/env python3
"""Writes tests/golden/tiff/: small TIFF files written by PIL (libtiff), and pixels.npz with what they hold.

    python tests/golden/make_tiff_goldens.py

Needs Pillow with libtiff (written with Pillow 12.2.0, libtiff 4.7.1).  The tests only read the result.  A file is
<set>_<mode>.tif; its pixels are pixels.npz[<mode>], for lzw_reset_I16.tif pixels.npz["reset"].  Modes: L (uint8),
I16 (uint16), F (float32), RGB (uint8 x 3), all 37 x 53 -- with 5 rows per strip the last strip has 2 rows.

  strips1 / strips5        uncompressed, one strip / 5 rows per strip
  packbits / lzw / deflate 5 rows per strip, no predictor
  lzw_2 / deflate_2        Predictor 2, as PIL writes them (L, I16, RGB, F)
  lzw_3 / deflate_3        Predictor 3 (F)
  packbits_2 / raw_2       Predictor tag 2 present, data NOT differenced: libtiff's PackBits and raw codecs never
                           install the predictor (I16)
  lzw_reset                one 96 x 96 strip of full-entropy uint16: the 4094-entry table fills and a Clear occurs
                           mid-stream (asserted below)"""
import os

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "tiff")
H, W = 37, 53


def pixels():
    rng = np.random.default_rng(2013)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = 40.0 * np.sin(xx / 7.0) + 3.0 * yy
    return {
        "L": np.clip(ramp + 120 + rng.integers(0, 6, (H, W)), 0, 255).astype(np.uint8),
        "I16": (ramp * 90 + 9000 + rng.integers(0, 300, (H, W))).astype(np.uint16),
        "F": (ramp * 0.37 - 11.5 + rng.random((H, W))).astype(np.float32),  # negative values occur
        "RGB": np.clip(np.stack([ramp + 100, 200 - ramp, xx * 4.0], axis=2) + rng.integers(0, 9, (H, W, 3)), 0,
                       255).astype(np.uint8),
        "reset": rng.integers(0, 65536, (96, 96), dtype=np.uint16),
    }


def clear_codes(stream):
    """number of Clear codes in a TIFF LZW stream (walks the code widths only)"""
    bitpos, width, n, clears = 0, 9, 258, 0
    fresh = True
    while bitpos + width <= len(stream) * 8:
        at = bitpos >> 3
        code = (int.from_bytes(stream[at:at + 3].ljust(3, b"\0"), "big") >> (24 - (bitpos & 7) - width)) & ((1 << width) - 1)
        bitpos += width
        if code == 257:
            break
        if code == 256:
            clears, width, n, fresh = clears + 1, 9, 258, True
            continue
        if not fresh:
            n += 1
        fresh = False
        width = 9 + (n >= 511) + (n >= 1023) + (n >= 2047)
    return clears


def save(name, array, compression, rows=None, predictor=None):
    info = {}
    if rows:
        info[278] = rows
    if predictor:
        info[317] = predictor
    path = os.path.join(OUT, name + ".tif")
    Image.fromarray(array).save(path, compression=compression, tiffinfo=info)
    with Image.open(path) as im:
        back = np.array(im)
        if predictor:
            assert im.tag_v2[317] == predictor, name
        if rows:
            assert im.tag_v2[278] == rows and len(im.tag_v2[273]) == -(-array.shape[0] // rows), name
    assert back.dtype == array.dtype and np.array_equal(back, array), name
    return path


def main():
    os.makedirs(OUT, exist_ok=True)
    px = pixels()
    np.savez_compressed(os.path.join(OUT, "pixels.npz"), **px)
    for mode in ("L", "I16", "F", "RGB"):
        a = px[mode]
        save(f"strips1_{mode}", a, "raw")
        save(f"strips5_{mode}", a, "raw", rows=5)
        save(f"packbits_{mode}", a, "packbits", rows=5)
        save(f"lzw_{mode}", a, "tiff_lzw", rows=5)
        save(f"deflate_{mode}", a, "tiff_adobe_deflate", rows=5)
        save(f"lzw_2_{mode}", a, "tiff_lzw", predictor=2)
        save(f"deflate_2_{mode}", a, "tiff_adobe_deflate", predictor=2)
    save("lzw_3_F", px["F"], "tiff_lzw", predictor=3)
    save("deflate_3_F", px["F"], "tiff_adobe_deflate", predictor=3)
    save("packbits_2_I16", px["I16"], "packbits", rows=5, predictor=2)
    save("raw_2_I16", px["I16"], "raw", rows=5, predictor=2)
    path = save("lzw_reset_I16", px["reset"], "tiff_lzw")
    with Image.open(path) as im:
        (off,), (cnt,) = im.tag_v2[273], im.tag_v2[279]
    stream = open(path, "rb").read()[off:off + cnt]
    assert clear_codes(stream) >= 2, "the table never filled: no Clear inside the stream"
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"wrote {len(os.listdir(OUT))} files, {total} bytes, Pillow {Image.__version__}, "
          f"libtiff {features.version('libtiff')}")


if __name__ == "__main__":
    main()
