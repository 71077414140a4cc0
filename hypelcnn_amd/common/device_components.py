"""Connected regions of a mask on the compute device (csrc/components.hip): labelling, compaction of the labels to
0..n-1, the class votes of the pixels around every region, the relabelled target image, and the shadow-corrected scene
-- the launches utilities/reveal_shadow_targets.py is made of.  Rasters stay where they are: every function takes and
returns flat tensors on the backend's device; the one download is the component count, which sizes the vote table."""
import numpy
import torch

from hypelcnn_amd.backend import COMPACT_TILE, COMPONENTS_MAX_CLASSES, COMPONENTS_OK, HypelError, Ref
from hypelcnn_amd.common.device_scene import _Source


def _check_image(h, w):
    if h <= 0 or w <= 0:
        raise ValueError(f"device_components: empty image {h} x {w}")
    if h * w >= 2 ** 31:
        raise ValueError(f"device_components: image too large, h * w = {h * w} >= 2**31 (pixel indices are int32)")


def _check_classes(n_classes):
    if not 1 <= n_classes <= COMPONENTS_MAX_CLASSES:
        raise ValueError(f"device_components: n_classes = {n_classes} is outside 1..{COMPONENTS_MAX_CLASSES} "
                         f"(the excluded classes are a 64-bit mask)")


def label_components(backend, mask_d, h, w):
    """mask_d: uint8 [h * w] on the device, non-zero = inside.  -> root int32 [h * w]: the row-major index of the first
    pixel of every pixel's 8-connected component, -1 outside the mask."""
    h, w = int(h), int(w)
    _check_image(h, w)
    root, ws = backend.empty(h * w, torch.int32), backend.empty(h * w, torch.int32)
    status = backend.zeros(1, torch.int32)
    backend.call("components_label_u8", Ref(mask_d), h, w, Ref(root), Ref(ws), Ref(status))
    code = int(status.cpu()[0])
    if code != COMPONENTS_OK:
        raise HypelError(f"hypel_components_label_u8: status {code}: a walk to a root ran into its step cap")
    return root


def compact_components(backend, root, h, w):
    """-> (comp int32 [h * w]: the rank of every pixel's root among the roots in row-major order, -1 outside the mask;
    the number of components, downloaded)."""
    h, w = int(h), int(w)
    _check_image(h, w)
    comp, count = backend.empty(h * w, torch.int32), backend.zeros(1, torch.int32)
    ws = backend.empty((h * w + COMPACT_TILE - 1) // COMPACT_TILE, torch.int32)
    backend.call("components_compact_i32", Ref(root), h, w, Ref(comp), Ref(count), Ref(ws))
    return comp, int(count.cpu()[0])


def exclude_mask(classes):
    bits = 0
    for c in classes:
        if 0 <= int(c) < 64:
            bits |= 1 << int(c)
    return bits


def component_votes(backend, targets_d, comp, h, w, n_components, n_classes, exclude=()):
    """-> (votes int32 [n * n_classes], size int32 [n], winner uint8 [n]) on the device: the classes (below n_classes,
    not in `exclude`) of the pixels outside the mask around every component, counted once per component pixel they
    touch; the winner is the most frequent class, the smallest on a tie, 255 without a vote."""
    h, w, n, n_classes = int(h), int(w), int(n_components), int(n_classes)
    _check_image(h, w)
    _check_classes(n_classes)
    votes, size = backend.empty(max(n, 1) * n_classes, torch.int32), backend.empty(max(n, 1), torch.int32)
    winner = backend.empty(max(n, 1), torch.uint8)
    backend.call("components_votes_i32", Ref(targets_d), Ref(comp), h, w, n, n_classes, exclude_mask(exclude),
                 Ref(votes), Ref(size), Ref(winner))
    return votes[:n * n_classes], size[:n], winner[:n]


def relabel_components(backend, targets_d, comp, winner, h, w, plus_one=False):
    """-> uint8 [h * w]: targets with every component that has a winner painted in it; plus_one raises every value
    other than 255 by one (the stored form of the ground truth)."""
    h, w = int(h), int(w)
    _check_image(h, w)
    out = backend.empty(h * w, torch.uint8)
    if winner.numel() == 0:
        winner = backend.zeros(4, torch.uint8)  # no component: never read, but the pointer must be one
    backend.call("components_relabel_u8", Ref(targets_d), Ref(comp), Ref(winner), h, w, int(bool(plus_one)), Ref(out))
    return out


def shadow_correct(backend, raster, mask_d, ratio):
    """raster: [h, w, bands] of float32 / uint16 / int16 / uint8 -- a NumPy array (or view) or a tiff_io.DeviceRaster,
    read through its strides.  -> float32 [h * w * bands] = c + c * (m * (ratio - 1)), NumPy's float32 arithmetic."""
    src = raster if isinstance(raster, _Source) else _Source(backend, raster)
    _check_image(src.h, src.w)
    r_minus_1 = numpy.asarray(ratio, dtype=numpy.float32) - numpy.float32(1)
    if r_minus_1.shape != (src.bands,):
        raise ValueError(f"device_components: {r_minus_1.shape} ratios for {src.bands} bands")
    out = backend.empty(src.h * src.w * src.bands, torch.float32)
    r_d = backend.upload(r_minus_1)
    backend.call("shadow_correct_f32", src.ref, src.code, *src.geometry(), Ref(mask_d), Ref(r_d), Ref(out))
    backend.synchronize()  # the uploaded operands are released when this returns
    return out
