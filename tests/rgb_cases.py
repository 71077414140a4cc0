"""TEST SUPPORT for the sRGB rendering (hypelcnn_amd/common/hsi_rgb_converter.py, hypel_hsi_to_srgb): the float64
NumPy oracle, written from the specification (reference common/hsi_rgb_converter.py get_rgb_from_hsi with colour-science's
CIE 1931 2 degree observer under illuminant E and scikit-image's xyz2rgb) and never from the package; the same chain in
float32, which measures what float32 arithmetic costs on a test's own inputs; the emulation of the kernel; the raster
builder of the device tests and the pass rule."""
import numpy as np

from hypelcnn_amd.backend import OUT_DTYPES, RGB_F32
from tests.emu_backend import _arr
from tests.test_gan_inference import DenormEmu

# CIE 1931 2 degree observer, 400 ... 700 nm in 10 nm steps, xbar ybar zbar per row (the CIE's published table)
CMF = np.array("""
0.014310 0.000396 0.067850  0.043510 0.001210 0.207400  0.134380 0.004000 0.645600  0.283900 0.011600 1.385600
0.348280 0.023000 1.747060  0.336200 0.038000 1.772110  0.290800 0.060000 1.669200  0.195360 0.090980 1.287640
0.095640 0.139020 0.812950  0.032010 0.208020 0.465180  0.004900 0.323000 0.272000  0.009300 0.503000 0.158200
0.063270 0.710000 0.078250  0.165500 0.862000 0.042160  0.290400 0.954000 0.020300  0.433450 0.994950 0.008750
0.594500 0.995000 0.003900  0.762100 0.952000 0.002100  0.916300 0.870000 0.001650  1.026300 0.757000 0.001100
1.062200 0.631000 0.000800  1.002600 0.503000 0.000340  0.854450 0.381000 0.000190  0.642400 0.265000 0.000050
0.447900 0.175000 0.000020  0.283500 0.107000 0         0.164900 0.061000 0         0.087400 0.032000 0
0.046770 0.017000 0         0.022700 0.008210 0         0.011359 0.004102 0
""".split(), dtype=np.float64).reshape(31, 3)
XYZ_FROM_RGB = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
KNEE = 0.0031308  # linear value at which the sRGB curve leaves its straight piece
U8_MAX_DIFF, U8_MAX_SHARE = 1, 1e-3  # the pass rule of a uint8 rendering


def oracle_select(band_measurements):
    """Band selection as the specification words it: the measurements are rounded; for each of 400, 410 ... 700 nm an
    explicit walk over the bands keeps the first index at which the distance to that wavelength is smallest."""
    rounded = [float(np.round(m)) for m in band_measurements]
    picks = []
    for wavelength in range(400, 701, 10):
        best, best_distance = 0, abs(rounded[0] - wavelength)
        for index in range(1, len(rounded)):
            distance = abs(rounded[index] - wavelength)
            if distance < best_distance:  # strictly: a later band at the same distance does not replace the first
                best, best_distance = index, distance
        picks.append(best)
    return picks


def _chain(band_measurements, r, ft):
    """get_rgb_from_hsi on normalised reflectance r [..., bands], every operation in the float type ft."""
    cmf = CMF.astype(ft)
    spectral = r[..., oracle_select(band_measurements)].astype(ft)
    s, dw = ft(1.0), ft(10.0)  # illuminant E, 10 nm
    k = ft(100.0) / (np.sum(cmf[:, 1] * s) * dw)
    xyz = k * np.sum(spectral[..., None] * cmf * s * dw, axis=-2)
    return _curve((xyz / ft(100.0)) @ np.linalg.inv(XYZ_FROM_RGB).T.astype(ft), ft)


def _curve(lin, ft):
    """scikit-image's transfer curve and clip on linear sRGB."""
    with np.errstate(invalid="ignore"):
        rgb = np.where(lin > ft(KNEE), ft(1.055) * np.power(lin, ft(1.0) / ft(2.4)) - ft(0.055), ft(12.92) * lin)
    assert rgb.dtype == ft
    return np.clip(rgb, ft(0.0), ft(1.0))


def oracle_rgb_of_linear(lin):
    return _curve(np.asarray(lin, np.float64), np.float64)


def oracle_rgb(band_measurements, r):
    """float64 sRGB in [0, 1] of normalised reflectance r [..., bands]."""
    return _chain(band_measurements, np.asarray(r, np.float64), np.float64)


def float32_rgb(band_measurements, r):
    """The same chain with every operation in float32: its distance from oracle_rgb is what the number format costs."""
    return _chain(band_measurements, np.asarray(r, np.float32), np.float32)


def normalise(raster, casi_min, casi_max, ft=np.float64):
    """The reference CLI's re-normalisation of the quantised raster: (raster.astype(float) - casi_min) / casi_max."""
    return (raster.astype(ft) - np.asarray(casi_min).astype(ft)) / np.asarray(casi_max).astype(ft)


def oracle_u8(band_measurements, raster, casi_min, casi_max):
    """What the reference CLI writes: (rgb * 255).astype(uint8) of the re-normalised raster; the cast truncates."""
    return (oracle_rgb(band_measurements, normalise(raster, casi_min, casi_max)) * 255).astype(np.uint8)


def check_u8(got, want):
    """The pass rule of a uint8 rendering; returns the share of samples that differ at all."""
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    share = float((diff != 0).mean())
    print(f"\nu8 rendering: {diff.size} samples, share differing {share:.3e}, largest difference {int(diff.max())}")
    assert diff.max() <= U8_MAX_DIFF, int(diff.max())
    assert share <= U8_MAX_SHARE, share
    return share


class RgbEmu(DenormEmu):
    def k_hsi_to_srgb(self, raster, in_dtype, ld_in, n_pixels, bands, band0, span, table, levels, out_mode, out):
        """include/hypel.h hypel_hsi_to_srgb: XYZ = sum_b (raster[p][band0 + b] - table[b][0]) * table[b][1:4] and the
        inverse sRGB matrix in float64; float32 output from the float32 transfer curve and clip; uint8 output = the
        largest k with levels[k] <= lin; non-finite values render as 0."""
        assert 0 <= band0 and 0 < span <= bands - band0 and bands <= ld_in
        dtype = {v: k for k, v in OUT_DTYPES.items()}[int(in_dtype)]
        flat = raster.t.numpy().view(np.uint8)[raster.off * raster.t.element_size():].view(dtype)
        rows = np.lib.stride_tricks.as_strided(flat[band0:], shape=(n_pixels, span),
                                               strides=(ld_in * dtype.itemsize, dtype.itemsize))
        t = _arr(table, np.float64)[: span * 4].reshape(span, 4)
        with np.errstate(invalid="ignore", over="ignore"):
            xyz = (rows.astype(np.float64) - t[:, 0]) @ t[:, 1:]
            lin = xyz @ np.linalg.inv(XYZ_FROM_RGB).T
            finite = np.isfinite(lin)
            if int(out_mode) == RGB_F32:
                l32 = lin.astype(np.float32)
                rgb = np.where(l32 > np.float32(KNEE),
                               np.float32(1.055) * np.power(l32, np.float32(1.0) / np.float32(2.4)) - np.float32(0.055),
                               np.float32(12.92) * l32)
                rgb = np.where(finite, np.clip(rgb, np.float32(0.0), np.float32(1.0)), np.float32(0.0))
                _arr(out)[: n_pixels * 3] = rgb.reshape(-1)
            else:
                lv = _arr(levels, np.float64)[:256]
                assert lv[0] == -np.inf and (np.diff(lv) > 0).all()
                k = np.searchsorted(lv, np.where(finite, lin, -1.0), side="right") - 1
                _arr(out, np.uint8)[: n_pixels * 3] = k.astype(np.uint8).reshape(-1)


# ----------------------------------------------------------------------------- rasters of the device tests
def measurements(bands):
    """Band wavelengths per band count: the real sensors' where the count is one of theirs."""
    return {8: np.linspace(400, 700, 8), 31: np.linspace(400, 700, 31), 48: np.linspace(380, 1050, 48),
            144: np.linspace(380, 1050, 144), 360: np.linspace(400, 2500, 360)}[bands]


def normalisation(dtype, bands, per_band, rng):
    """(casi_min, casi_max) as a loader holds them: of the scene's dtype, scalar or one per band."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        lo, hi = (rng.random(bands) * 0.2 - 0.1).astype(np.float32), (0.8 + rng.random(bands)).astype(np.float32)
    else:
        top = np.iinfo(dtype).max
        lo = rng.integers(0, top // 16, bands).astype(dtype)
        hi = (top - lo.astype(np.int64) - rng.integers(0, top // 8, bands)).astype(dtype)
    return (lo, hi) if per_band else (lo[0], hi[0])


def edge_raster(h, w, bands, ld_in, dtype, casi_min, casi_max, rng):
    """[h * w, ld_in] raster of `dtype`: smooth random spectra, and rows built for the edges of the curve -- grey levels
    whose linear value lies on either side of the knee, saturated spectra (one narrow line: linear sRGB goes negative
    and clips to 0), reflectance above 1 (clips to 1), all-zero rows, the dtype's full scale.  The padding columns
    hold a value that would show in the rendering if it were read."""
    dtype = np.dtype(dtype)
    n = h * w
    lo = np.broadcast_to(np.asarray(casi_min, np.float64), (bands,))
    hi = np.broadcast_to(np.asarray(casi_max, np.float64), (bands,))
    x = np.linspace(0, 1, bands)
    a, c, s = rng.random((3, n, 1))
    r = np.clip(0.05 + 0.9 * a * np.exp(-((x - c) / (0.15 + s)) ** 2) + 0.02 * rng.standard_normal((n, bands)), 0, 1)
    grey = KNEE * np.array([0.5, 0.9, 0.99, 1.01, 1.1, 2.0, 0.0])
    r[: grey.size] = grey[:, None]
    k = grey.size
    for j, b in enumerate(np.linspace(0, bands - 1, 6).astype(int)):  # narrow lines across the spectrum
        r[k + j] = 0.0
        r[k + j, b] = 1.0
    k += 6
    r[k: k + 3] = np.array([1.5, 4.0, 1.0])[:, None]
    k += 3
    v = r * hi + lo
    if dtype == np.float32:
        raster = v.astype(np.float32)
        raster[k] = 0.0
        full, pad = np.float32(3.0), np.float32(1e6)
    else:
        info = np.iinfo(dtype)
        raster = np.clip(np.round(v), info.min, info.max).astype(dtype)
        raster[k] = 0
        full, pad = info.max, info.max
        if info.min < 0:
            raster[k + 2] = info.min
    raster[k + 1] = full
    assert k + 3 <= n
    out = np.full((n, ld_in), pad, dtype)
    out[:, :bands] = raster
    return out
