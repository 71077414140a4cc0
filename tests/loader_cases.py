"""TEST INFRASTRUCTURE: the small seeded data directories the loader tests and tests/golden/make_reference_loaders.py
share -- one writer, so that a test regenerates byte-identical files without the reference.

Geometry: 24 x 31 pixels.  GRSS2013: 16 float32 bands + float32 LiDAR.  GULFPORT: 12 uint16 bands + uint16 LiDAR, with
the shadowed / deshadowed companions.  AVON: 12 uint16 bands stored [band, column, row + 110 blank], heavy upper tails
so that the 95th-percentile clip changes values in every band; target masks as BMP with 110 blank rows."""
import os
import struct

import numpy as np

from hypelcnn_amd.common.tiff_io import imwrite

H, W = 24, 31
NEIGHBORHOOD = 2
BLANK = 55
BANDS = {"GRSS2013DataLoader": 16, "GULFPORTDataLoader": 12, "GULFPORTALTDataLoader": 12, "AVONDataLoader": 12}
LOADERS = tuple(BANDS)
# (x, y) in scene coordinates: the four corners first
POINTS = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (1, 1), (15, 12), (7, 20), (30, 11), (12, 0), (0, 9),
          (22, 5), (3, 17)]


def write_bmp(path, image, top_down=False):
    """bool [H, W] -> 1 bit per pixel (palette black, white); uint8 [H, W] -> 8 bits with a gray ramp; uint8
    [H, W, 3] -> 24 bits.  Rows are padded to four bytes; bottom-up unless top_down."""
    img = np.asarray(image)
    h, w = img.shape[:2]
    if img.dtype == bool:
        bits, palette = 1, bytes([0, 0, 0, 0, 255, 255, 255, 0])
        rows = np.packbits(img, axis=1)
    elif img.ndim == 2:
        bits, palette = 8, b"".join(bytes([i, i, i, 0]) for i in range(256))
        rows = img.astype(np.uint8)
    else:
        bits, palette = 24, b""
        rows = img[:, :, ::-1].reshape(h, w * 3).astype(np.uint8)
    stride = ((w * bits + 31) // 32) * 4
    lines = np.zeros((h, stride), np.uint8)
    lines[:, :rows.shape[1]] = rows
    if not top_down:
        lines = lines[::-1]
    off = 54 + len(palette)
    with open(path, "wb") as f:
        f.write(b"BM" + struct.pack("<IHHI", off + stride * h, 0, 0, off))
        f.write(struct.pack("<IiiHHIIiiII", 40, w, -h if top_down else h, 1, bits, 0, stride * h, 2835, 2835,
                            len(palette) // 4, 0))
        f.write(palette + lines.tobytes())


def _labels(rng, classes, first, fill, share=0.45):
    """uint8 [H, W]: `share` of the pixels carry a class first .. first + classes - 1, the others `fill`; every class
    occurs at least four times"""
    lab = np.full(H * W, fill, np.uint8)
    pick = rng.permutation(H * W)[: int(H * W * share)]
    lab[pick] = first + np.arange(pick.size) % classes
    return lab.reshape(H, W)


def _shadow_map(rng):
    smap = np.zeros((H, W), np.uint8)
    smap[5:14, 8:21] = 1
    smap[rng.random((H, W)) < 0.05] = 1
    return smap


def write_data_dir(base):
    """Writes <base>/2013_DFTC, <base>/GULFPORT and <base>/AVON.  Returns base."""
    rng = np.random.default_rng(20130)
    d = os.path.join(base, "2013_DFTC")
    os.makedirs(d, exist_ok=True)
    smap = _shadow_map(rng)
    casi = (rng.random((H, W, 16)) * 9000 + 300 + 700 * np.arange(16)).astype(np.float32)
    casi = np.where(smap[..., None] == 1, casi * (0.3 + 0.02 * np.arange(16)), casi).astype(np.float32)
    casi[3, 4, :] = -12.5  # negative floats occur
    imwrite(os.path.join(d, "2013_IEEE_GRSS_DF_Contest_CASI.tif"), casi)
    imwrite(os.path.join(d, "2013_IEEE_GRSS_DF_Contest_LiDAR.tif"), (rng.random((H, W)) * 40 + 3).astype(np.float32))
    imwrite(os.path.join(d, "shadow_map.tif"), smap)
    imwrite(os.path.join(d, "2013_IEEE_GRSS_DF_Contest_Samples_TR.tif"), _labels(rng, 15, 0, 255, 0.4))
    imwrite(os.path.join(d, "2013_IEEE_GRSS_DF_Contest_Samples_VA.tif"), _labels(rng, 15, 0, 255, 0.3))

    rng = np.random.default_rng(11)
    d = os.path.join(base, "GULFPORT")
    os.makedirs(d, exist_ok=True)
    smap = _shadow_map(rng)
    hsi = np.rint(rng.random((H, W, 12)) * 3000 + 400 + 100 * np.arange(12))
    hsi = np.where(smap[..., None] == 1, hsi * 0.4, hsi)
    imwrite(os.path.join(d, "muulf_hsi.tif"), np.rint(hsi).astype(np.uint16))
    # the converted scenes leave the original's range on both sides: the original's extrema still normalise them
    imwrite(os.path.join(d, "muulf_hsi_shadowed.tif"), np.rint(hsi * 0.5 + 20).astype(np.uint16))
    imwrite(os.path.join(d, "muulf_hsi_deshadowed.tif"), np.rint(hsi * 1.7 + 50).astype(np.uint16))
    imwrite(os.path.join(d, "muulf_lidar.tif"), np.rint(rng.random((H, W)) * 500 + 7).astype(np.uint16))
    imwrite(os.path.join(d, "muulf_shadow_map.tif"), smap)
    imwrite(os.path.join(d, "muulf_gt.tif"), _labels(rng, 11, 1, 0, 0.5))
    imwrite(os.path.join(d, "muulf_gt_shadow_corrected.tif"), _labels(rng, 11, 1, 0, 0.6))

    rng = np.random.default_rng(360)
    d = os.path.join(base, "AVON")
    os.makedirs(d, exist_ok=True)
    smap = _shadow_map(rng)
    scene = rng.random((H, W, 12)) * 2500 + 150 + 40 * np.arange(12)
    scene = np.where(smap[..., None] == 1, scene * 0.35, scene)
    tail = rng.random((H, W, 12)) < 0.09  # more than 5 % of every band lies far above the rest
    scene = np.rint(np.where(tail, scene * (4 + 11 * rng.random((H, W, 12))), scene)).astype(np.uint16)
    stored = np.zeros((12, W, H + 2 * BLANK), np.uint16)
    stored[:, :, BLANK:-BLANK] = scene.transpose(2, 1, 0)
    stored[:, :, :BLANK] = 60000  # the blank margin must not leak into any statistic
    imwrite(os.path.join(d, "0920-1857.georef_cropped.tif"), stored)
    imwrite(os.path.join(d, "0920-1857.georef_cropped_shcorrected.tif"),
            np.rint(scene * 1.1 + 5).clip(0, 65535).astype(np.uint16))
    imwrite(os.path.join(d, "0920-1857.georef_cropped_shadow.tif"), smap)
    for no in (1, 2):
        marks = rng.random((H, W)) < 0.2
        for kind, sel in (("nsh", marks & (smap == 0)), ("sh", marks & (smap == 1))):
            mask = np.zeros((H + 2 * BLANK, W), bool)
            mask[BLANK:-BLANK] = sel
            path = os.path.join(d, f"0920-1857.georef_cropped_rgb_with_targets_{no}_{kind}.bmp")
            if kind == "nsh":
                write_bmp(path, mask, top_down=(no == 2))  # 1 bit: the loader's bool branch
            else:
                write_bmp(path, mask.astype(np.uint8) * 255)  # 8 bit gray
    return base
