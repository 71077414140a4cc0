"""sRGB rendering of a hyperspectral scene (reference common/hsi_rgb_converter.py), on the device.

The reference picks the 31 bands nearest to 400, 410 ... 700 nm, weighs them with the CIE 1931 2 degree colour matching
functions under illuminant E (colour-science), and converts XYZ to sRGB with scikit-image's xyz2rgb.  Neither library
is needed: the conversion is the 93 published constants below, one 3x3 matrix and the sRGB transfer curve.  The band
selection and the weights are host work of a few hundred numbers; the pass over the raster is one hypel_hsi_to_srgb
launch (csrc/data.hip).  There is no CPU path.

The colour matching functions are typed from the CIE's published table; no copy of colour-science was at hand to hold
them against, so tests/test_hsi_rgb.py pins their column sums and the rendering of a flat spectrum."""
import functools

import numpy
import torch

from hypelcnn_amd.backend import OUT_DTYPES, RGB_F32, RGB_U8, Ref

VISUAL_SPECTRUM = tuple(range(400, 701, 10))

# CIE 1931 2 degree standard observer, xbar ybar zbar at 400, 410 ... 700 nm
CIE1931_2 = numpy.array([
    [0.014310, 0.000396, 0.067850], [0.043510, 0.001210, 0.207400], [0.134380, 0.004000, 0.645600],
    [0.283900, 0.011600, 1.385600], [0.348280, 0.023000, 1.747060], [0.336200, 0.038000, 1.772110],
    [0.290800, 0.060000, 1.669200], [0.195360, 0.090980, 1.287640], [0.095640, 0.139020, 0.812950],
    [0.032010, 0.208020, 0.465180], [0.004900, 0.323000, 0.272000], [0.009300, 0.503000, 0.158200],
    [0.063270, 0.710000, 0.078250], [0.165500, 0.862000, 0.042160], [0.290400, 0.954000, 0.020300],
    [0.433450, 0.994950, 0.008750], [0.594500, 0.995000, 0.003900], [0.762100, 0.952000, 0.002100],
    [0.916300, 0.870000, 0.001650], [1.026300, 0.757000, 0.001100], [1.062200, 0.631000, 0.000800],
    [1.002600, 0.503000, 0.000340], [0.854450, 0.381000, 0.000190], [0.642400, 0.265000, 0.000050],
    [0.447900, 0.175000, 0.000020], [0.283500, 0.107000, 0.000000], [0.164900, 0.061000, 0.000000],
    [0.087400, 0.032000, 0.000000], [0.046770, 0.017000, 0.000000], [0.022700, 0.008210, 0.000000],
    [0.011359, 0.004102, 0.000000]], dtype=numpy.float64)

_OTHER_OBSERVERS = ("cie1964_10", "cie2012_2", "cie2012_10")  # named by the reference, never used by it


def get_cmfs(cmf_name="cie1931_2"):
    """[31, 3] colour matching functions at VISUAL_SPECTRUM (reference _get_cmfs with split=False)."""
    if cmf_name == "cie1931_2":
        return CIE1931_2
    if cmf_name in _OTHER_OBSERVERS:
        raise NotImplementedError(f"observer {cmf_name} is not built: the rendering uses cie1931_2 only")
    raise AttributeError("Wrong cmf name")


def select_visual_bands(band_measurements):
    """For 400, 410 ... 700 nm the first band whose rounded wavelength is nearest (reference get_rgb_from_hsi :66-71).
    Duplicates are legal (few bands), and so are picks far outside the visual range (a scene that starts above it)."""
    wi = numpy.round(numpy.asarray(band_measurements, numpy.float64))
    return [int(numpy.argmin(numpy.abs(wi - i))) for i in VISUAL_SPECTRUM]


def _levels_u8(lin):
    """What the reference writes for a linear sRGB value, float64: the curve, the clip, (rgb * 255).astype(uint8)."""
    lin = numpy.asarray(lin, numpy.float64)
    with numpy.errstate(invalid="ignore"):
        rgb = numpy.where(lin > 0.0031308, 1.055 * numpy.power(lin, 1 / 2.4) - 0.055, 12.92 * lin)
    return (numpy.clip(rgb, 0, 1) * 255).astype(numpy.uint8)


@functools.lru_cache(maxsize=None)
def srgb_levels():
    """levels [256] float64 of hypel_hsi_to_srgb's byte output: levels[0] = -inf, levels[k] = the smallest float64 linear
    value that the reference's float64 expression renders as k.  The inverse of the curve lands within a few units in
    the last place of it; the expression itself then settles which neighbour is the first to reach k."""
    k = numpy.arange(1, 256, dtype=numpy.float64)
    srgb = k / 255
    lin = numpy.where(srgb > 12.92 * 0.0031308, ((srgb + 0.055) / 1.055) ** 2.4, srgb / 12.92)
    for _ in range(64):  # down while the value below still renders as k, up while this one does not yet
        below = numpy.nextafter(lin, -numpy.inf)
        down, up = _levels_u8(below) >= k, _levels_u8(lin) < k
        if not (down | up).any():
            break
        lin = numpy.where(down, below, numpy.where(up, numpy.nextafter(lin, numpy.inf), lin))
    else:
        raise AssertionError("srgb_levels did not settle")
    levels = numpy.concatenate([[-numpy.inf], lin])
    levels.setflags(write=False)
    return levels


def render_table(band_measurements, bands, scale=None, offset=None, cmf_name="cie1931_2"):
    """(band0, span, table [span, 4] float64) of hypel_hsi_to_srgb: row b = {offset, wx, wy, wz} of band band0 + b.

    The 31 picks are folded into one weight per band of the span they cover (a band picked twice weighs twice, a band
    never picked weighs zero), together with 1 / sum(ybar) -- illuminant E and the 10 nm step cancel in the reference's
    k * sum(r * cmf * s * dw) / 100 -- and with 1 / scale of r = (v - offset) / scale.  The span is widened to
    four-band boundaries where the scene has the bands, so that rows of a four-aligned raster load four bands a lane."""
    cmfs = get_cmfs(cmf_name)
    sel = numpy.asarray(select_visual_bands(band_measurements))
    if sel.max() >= bands:
        raise ValueError(f"band_measurements name {sel.max() + 1} bands, the raster has {bands}")
    weights = numpy.zeros((bands, 3), numpy.float64)
    numpy.add.at(weights, sel, cmfs / cmfs[:, 1].sum())
    scale = numpy.broadcast_to(numpy.asarray(1.0 if scale is None else scale, numpy.float64), (bands,))
    offset = numpy.broadcast_to(numpy.asarray(0.0 if offset is None else offset, numpy.float64), (bands,))
    picked = weights.any(axis=1)
    weights[picked] /= scale[picked, None]
    band0 = int(sel.min()) // 4 * 4
    end = min((int(sel.max()) + 4) // 4 * 4, bands)
    table = numpy.concatenate([numpy.where(picked, offset, 0.0)[band0:end, None], weights[band0:end]], axis=1)
    return band0, end - band0, numpy.ascontiguousarray(table)


def launch_render(backend, raster, dtype, ld_in, n_pixels, bands, band_measurements, scale, offset, out_mode):
    """One hypel_hsi_to_srgb launch over raster (a Ref to [n_pixels, ld_in] of dtype); the flat device output."""
    dtype = numpy.dtype(dtype)
    if dtype not in OUT_DTYPES:
        raise ValueError(f"raster dtype {dtype} is not supported by the sRGB rendering (float32, uint16, int16, uint8)")
    band0, span, table = render_table(band_measurements, bands, scale, offset)
    out = backend.empty(n_pixels * 3, torch.uint8 if out_mode == RGB_U8 else torch.float32)
    levels = Ref(backend.upload(srgb_levels())) if out_mode == RGB_U8 else None
    backend.call("hsi_to_srgb", raster, OUT_DTYPES[dtype], ld_in, n_pixels, bands, band0, span,
                 Ref(backend.upload(table)), levels, out_mode, Ref(out))
    return out


def render_raster_rgb(backend, raster_dev, dtype, h, w, bands, band_measurements, casi_min, casi_max):
    """uint8 [h, w, 3]: (get_rgb_from_hsi(band_measurements, (raster - casi_min) / casi_max) * 255).astype(uint8) of
    the device raster [h * w, bands] of `dtype` (a flat tensor of any element type), as the reference's CLI renders the
    converted scene (gan/gan_infer_image_for_shadow.py:97-104)."""
    out = launch_render(backend, Ref(raster_dev), dtype, bands, h * w, bands, band_measurements, casi_max, casi_min,
                        RGB_U8)
    backend.synchronize()
    return out.cpu().numpy().reshape(h, w, 3)


def get_rgb_from_hsi(band_measurements, casi_normalized, backend=None):
    """float32 sRGB [H, W, 3] in [0, 1] of the normalised scene [H, W, bands] (reference get_rgb_from_hsi).  A NumPy
    array is uploaded and the rendering comes back as one; a tensor is rendered where it is and a tensor returned."""
    if backend is None:
        from hypelcnn_amd.backend import HipBackend
        backend = HipBackend()
    h, w, bands = casi_normalized.shape
    if isinstance(casi_normalized, torch.Tensor):
        flat = casi_normalized.to(device=backend.device, dtype=torch.float32).contiguous().reshape(-1)
    else:
        flat = backend.upload(numpy.asarray(casi_normalized, numpy.float32))
    out = launch_render(backend, Ref(flat), numpy.float32, bands, h * w, bands, band_measurements, None, None, RGB_F32)
    backend.synchronize()
    out = out.reshape(h, w, 3)
    return out if isinstance(casi_normalized, torch.Tensor) else out.cpu().numpy()
