"""Where a template raster lies inside an image raster, on the compute device (csrc/match.hip): what
cv2.matchTemplate(image, template, TM_CCORR_NORMED) followed by cv2.minMaxLoc's max_loc gives on rasters that
cv2.resize(..., INTER_AREA) enlarged by integer factors, which is pixel replication.  The enlarged rasters are never
built: the launches divide their coordinates by the scale.  Restated from OpenCV's documented formulas;
cv2 itself was never available to pin it against.

Rasters stay where they are: a NumPy array is uploaded (a band of a contiguous pixel-major scene as that scene, read in
place through its strides), a torch tensor on the backend's device is read through its strides.  The one download is
the 16-byte result record."""
import numpy
import torch

from hypelcnn_amd.backend import (MATCH_BLOCK_COLS, MATCH_COL_CHUNK, MATCH_MAX_SPLITS, MATCH_ROW_CHUNK, MATCH_TILE, OUT_DTYPES,
                                  Ref)
from hypelcnn_amd.common.device_scene import EXTREMA_SLICES, resident_view

LIMIT = 2 ** 31
# hypel_match_ccorr_f32's splits.  Measured at the contest geometry (NOTES.md, "Template matching"): the launch gets
# faster up to about 64 blocks per compute unit (its blocks share the SIMDs unevenly, so few long blocks leave a tail)
# and is flat beyond; a block should still have a few staged chunks to amortise its first fetch and its output.
TARGET_BLOCKS = 16384
MIN_UNITS_PER_SPLIT = 16
MAX_PARTIAL_FLOATS = 1 << 26  # 256 MiB of partial surfaces


def _integer_scale(scale, what):
    if isinstance(scale, (bool, numpy.bool_)) or scale != int(scale):
        raise NotImplementedError(f"device_match: {what} scale {scale!r} is not an integer: only enlargement by an "
                                  f"integer factor >= 1 (pixel replication, what INTER_AREA does there) is built")
    if int(scale) < 1:
        raise NotImplementedError(f"device_match: {what} scale {scale!r} is below 1: shrinking rasters is not built, "
                                  f"only enlargement by an integer factor >= 1")
    return int(scale)


class _Band:
    """One float32 band in device memory, as the kernels address it: Ref to its first sample, (h, w), element strides,
    replication scale."""

    def __init__(self, backend, array, scale, what):
        self.what = what
        self.scale = _integer_scale(scale, what)
        if isinstance(array, torch.Tensor):
            if array.dim() != 2 or array.dtype != torch.float32 or 0 in array.shape:
                raise ValueError(f"device_match: the {what} must be a non-empty 2-D float32 raster")
            if array.device.type != torch.device(backend.device).type:
                raise ValueError(f"device_match: the {what} lives on another device than the backend")
            self.h, self.w = (int(v) for v in array.shape)
            strides = tuple(int(s) for s in array.stride())
            if any(n > 1 and s <= 0 for n, s in zip(array.shape, strides)):
                raise ValueError(f"device_match: the {what} has a non-positive stride")
            self.sy, self.sx = (0 if n == 1 else s for n, s in zip(array.shape, strides))
            span = (self.h - 1) * self.sy + (self.w - 1) * self.sx + 1
            self.flat = array.as_strided((span,), (1,), array.storage_offset())  # its window of the storage, no copy
            self.ref = Ref(self.flat)
        else:
            a = numpy.asarray(array)
            if a.ndim != 2 or 0 in a.shape:
                raise ValueError(f"device_match: the {what} must be a non-empty 2-D raster")
            root, offset, (self.sy, self.sx) = resident_view(a, numpy.float32, root_limit=LIMIT)
            self.h, self.w = (int(v) for v in a.shape)
            self.flat = backend.upload(root)
            self.ref = Ref(self.flat, offset)
        self.H, self.W = self.h * self.scale, self.w * self.scale
        if self.H * self.W >= LIMIT:
            raise ValueError(f"device_match: the enlarged {what} has {self.H} x {self.W} = {self.H * self.W} pixels, "
                             f"the limit is 2**31 (pixel indices are int32)")

    def geometry(self):
        return (self.h, self.w, self.sy, self.sx, self.scale)


class MatchResult:
    """score: the best float32 R; top_left / bottom_right: (x, y) of the window in enlarged image pixels, as
    cv2.minMaxLoc's max_loc and the reference's top_left + (w, h); shape: (hout, wout) of the score surface; scores:
    that surface as a flat float32 device tensor (keep_scores=True), else None."""
    __slots__ = ("score", "top_left", "bottom_right", "shape", "scores", "index")

    def __init__(self, score, index, shape, template_shape, scores):
        self.score, self.index, self.shape, self.scores = float(score), int(index), tuple(shape), scores
        y, x = divmod(self.index, shape[1])
        self.top_left = (x, y)
        self.bottom_right = (x + template_shape[1], y + template_shape[0])

    def __repr__(self):
        return (f"MatchResult(score={self.score!r}, top_left={self.top_left}, bottom_right={self.bottom_right}, "
                f"shape={self.shape})")


def choose_splits(hout, wout, ht, wt):
    """How many blocks share the template for one output tile: enough for TARGET_BLOCKS blocks, each with at least
    MIN_UNITS_PER_SPLIT (column chunk, row chunk) pairs, within MAX_PARTIAL_FLOATS of workspace."""
    blocks = -(-wout // MATCH_BLOCK_COLS) * -(-hout // MATCH_TILE)
    units = -(-wt // MATCH_COL_CHUNK) * -(-(MATCH_TILE - 1 + ht) // MATCH_ROW_CHUNK)
    splits = max(1, min(units // MIN_UNITS_PER_SPLIT, TARGET_BLOCKS // blocks, MATCH_MAX_SPLITS,
                        MAX_PARTIAL_FLOATS // (hout * wout)))
    return -(-units // -(-units // splits))  # no split without a pair


def window_energy(backend, band, win_h, win_w):
    """-> float64 [hout * wout] on the device: the sum of the enlarged band's squares over every win_h x win_w window"""
    hout, wout = band.H - win_h + 1, band.W - win_w + 1
    energy = backend.empty(hout * wout, torch.float64)
    ws = backend.empty(band.h * wout, torch.float64)
    backend.call("match_window_energy_f64", band.ref, *band.geometry(), win_h, win_w, Ref(energy), Ref(ws))
    return energy


def match_template(backend, image, template, image_scale=1, template_scale=1, keep_scores=False, splits=None):
    """image, template: 2-D float32 rasters (NumPy arrays or tensors on the backend's device, any positive strides),
    finite.  Each is enlarged by its integer scale first.  -> MatchResult of the best normalised cross-correlation."""
    img = image if isinstance(image, _Band) else _Band(backend, image, image_scale, "image")
    tpl = template if isinstance(template, _Band) else _Band(backend, template, template_scale, "template")
    if tpl.H > img.H or tpl.W > img.W:
        raise ValueError(f"device_match: the enlarged template ({tpl.H} x {tpl.W}) is larger than the enlarged image "
                         f"({img.H} x {img.W})")
    hout, wout = img.H - tpl.H + 1, img.W - tpl.W + 1
    splits = choose_splits(hout, wout, tpl.H, tpl.W) if splits is None else int(splits)
    if not 1 <= splits <= MATCH_MAX_SPLITS or hout * wout * splits >= LIMIT:
        raise ValueError(f"device_match: splits = {splits} is outside 1..{MATCH_MAX_SPLITS} or its partial surfaces "
                         f"reach 2**31 elements")
    num = backend.empty(hout * wout, torch.float32)
    ws = backend.empty(splits * hout * wout, torch.float32) if splits > 1 else None
    backend.call("match_ccorr_f32", img.ref, *img.geometry(), tpl.ref, *tpl.geometry(), Ref(num),
                 None if ws is None else Ref(ws), splits)
    energy = window_energy(backend, img, tpl.H, tpl.W)
    e_t = window_energy(backend, tpl, tpl.H, tpl.W)
    scores = backend.empty(hout * wout, torch.float32) if keep_scores else None
    record = backend.empty(2, torch.int64)
    backend.call("match_best_f32", Ref(num), Ref(energy), Ref(e_t), hout, wout,
                 None if scores is None else Ref(scores), Ref(record))
    raw = record.cpu().numpy()  # (synchronises: the uploaded operands may go when this returns)
    return MatchResult(raw.view(numpy.float32)[0], raw[1], (hout, wout), (tpl.H, tpl.W), scores)


def render_u8(backend, band):
    """-> uint8 [H * W] on the device: the enlarged band as grey levels, (v / max * 255) truncated, the reference's
    im_normalized raster.  The maximum comes from hypel_scene_extrema on the band as a one-band scene."""
    code = OUT_DTYPES[numpy.dtype(numpy.float32)]
    extrema = backend.zeros(2, torch.float32)
    ws = backend.empty(2 * EXTREMA_SLICES, torch.float32)
    backend.call("scene_extrema", band.ref, code, band.h, band.w, 1, band.sy, band.sx, 0, None, None, Ref(extrema),
                 Ref(extrema, 1), Ref(ws), EXTREMA_SLICES)
    out = backend.empty(band.H * band.W, torch.uint8)
    backend.call("match_render_u8", band.ref, *band.geometry(), Ref(extrema, 1), Ref(out))
    return out
