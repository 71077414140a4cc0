"""Extended morphological profiles for the classic-ML baselines: openings and closings (by reconstruction, or plain) of
the channels of a scene that is resident on the device as float32 pixels, at a ladder of structuring-element radii,
stacked as features -- the step published "PCA -> EMP -> SVM / RF" baselines put after the band PCA.  Four launches
(include/hypel.h, csrc/morph.hip): hypel_morph_keys_u32 maps floats to uint32 keys whose unsigned order is one total order
on float32 bit patterns, hypel_morph_erode_dilate_u32 and hypel_morph_reconstruct_sweep_u32 work on keys with integer
min / max, hypel_morph_profile_store_f32 turns keys back into floats inside the symmetric-padded stack.  Every output is
a bit copy of an input.

The reconstruction is driven from here: sweeps in groups of SWEEP_GROUP between two buffers, the device's `changed` word
read once per group, stop at the first group that leaves it clear (a sweep of a fixed point changes nothing, so the extra
sweeps of a group are no-ops).

Not here: attribute profiles, partial reconstruction, two-resolution scenes (GRSS2018), several scenes at
once (GULFPORTALT)."""
import numbers

import numpy as np
import torch

from hypelcnn_amd.backend import MORPH_DILATE, MORPH_DISK, MORPH_ERODE, MORPH_MAX_RADIUS, MORPH_SQUARE, Ref
from hypelcnn_amd.classic.decomposition import ProjectedScene

SHAPES = {"disk": MORPH_DISK, "square": MORPH_SQUARE}
METHODS = {"dilation": MORPH_DILATE, "erosion": MORPH_ERODE}
SWEEP_GROUP = 4


class MorphologicalProfile:
    """radii: strictly increasing integers in 1 .. MORPH_MAX_RADIUS, at least one (S of them).  shape: "disk" (offsets with
    dx^2 + dy^2 <= r^2) or "square".  by_reconstruction: opening gamma_r(f) = R^dilation_f(erode_r f), closing phi_r(f) =
    R^erosion_f(dilate_r f); False: the plain dilate_r erode_r f and erode_r dilate_r f.  The profile of a base image f is
    the 2 S + 1 channels [phi_rS .. phi_r1, f, gamma_r1 .. gamma_rS]; base b of a raster fills channels b (2 S + 1) ..
    b (2 S + 1) + 2 S.  include_lidar (transform_scene): the LiDAR channels follow the HSI channels as further bases, and
    the result has no LiDAR raster of its own; False: the LiDAR raster passes through untouched.
    sweeps_: after transform / transform_scene, "<raster>/<opening|closing>/<radius>" -> sweeps launched for that level."""

    def __init__(self, radii, shape="disk", by_reconstruction=True, include_lidar=True, backend=None):
        try:
            radii = tuple(radii)
        except TypeError:
            radii = (radii,)
        if not radii or any(isinstance(r, bool) or not isinstance(r, numbers.Integral) for r in radii) or \
                any(not 1 <= r <= MORPH_MAX_RADIUS for r in radii) or any(b <= a for a, b in zip(radii, radii[1:])):
            raise ValueError(f"MorphologicalProfile: radii={radii!r}: at least one, strictly increasing integers in "
                             f"1 .. {MORPH_MAX_RADIUS} (HYPEL_MORPH_MAX_RADIUS)")
        if shape not in SHAPES:
            raise ValueError(f"MorphologicalProfile: shape={shape!r}: one of {tuple(SHAPES)}")
        self.radii, self.shape = tuple(int(r) for r in radii), shape
        self.by_reconstruction, self.include_lidar = bool(by_reconstruction), bool(include_lidar)
        self._be = backend
        self.sweeps_ = {}

    def get_params(self):
        return {"radii": list(self.radii), "shape": self.shape, "by_reconstruction": self.by_reconstruction,
                "include_lidar": self.include_lidar}

    def _backend(self):
        if self._be is None:
            from hypelcnn_amd.backend import HipBackend
            self._be = HipBackend()
        return self._be

    # ------------------------------------------------------------------------------------------------ views and keys
    def _view(self, image, what):
        """[h, w] or [h, w, c] (NumPy array: uploaded; device tensor: read in place through its strides) -> (flat tensor
        at the view's origin, h, w, c, stride_y, stride_x)"""
        be = self._backend()
        if isinstance(image, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(be.device)
        elif isinstance(image, torch.Tensor):
            t = image.to(be.device)
        else:
            raise ValueError(f"MorphologicalProfile.{what}: a NumPy array or a device tensor, got {type(image).__name__}")
        if t.dtype != torch.float32:
            t = t.float()
        if t.dim() == 2:
            t = t.unsqueeze(2)
        if t.dim() != 3 or min(t.shape) < 1:
            raise ValueError(f"MorphologicalProfile.{what}: an image as [h, w] or [h, w, channels], got {tuple(image.shape)}")
        h, w, c = (int(v) for v in t.shape)
        if (c > 1 and t.stride(2) != 1) or (w > 1 and t.stride(1) < c) or (h > 1 and t.stride(0) < c):
            t = t.contiguous()
        sx = int(t.stride(1)) if w > 1 else c
        sy = int(t.stride(0)) if h > 1 else max(w * sx, c)
        span = (h - 1) * sy + (w - 1) * sx + c
        return t.as_strided((span,), (1,)), h, w, c, sy, sx

    def _keys(self, view):
        be = self._backend()
        flat, h, w, c, sy, sx = view
        keys = be.empty(h * w * c, torch.int32)
        be.call("morph_keys_u32", Ref(flat), h, w, c, sy, sx, Ref(keys))
        return keys

    def _store(self, keys, h, w, c, pad, out, out_c, chan_offset, chan_step):
        self._backend().call("morph_profile_store_f32", Ref(keys), h, w, c, pad, Ref(out), out_c, chan_offset, chan_step)

    def _floats(self, keys, h, w, c, like, squeeze):
        """keys -> what the caller handed in: a NumPy array for one, a device tensor for one; [h, w] for [h, w]"""
        out = self._backend().empty(h * w * c)
        self._store(keys, h, w, c, 0, out, c, 0, 1)
        out = out.view(h, w) if squeeze else out.view(h, w, c)
        return out.cpu().numpy() if isinstance(like, np.ndarray) else out

    def _erode_dilate(self, keys, h, w, c, radius, op):
        be = self._backend()
        out = be.empty(h * w * c, torch.int32)
        be.call("morph_erode_dilate_u32", Ref(keys), h, w, c, int(radius), SHAPES[self.shape], op, Ref(out))
        return out

    def _reconstruct(self, marker, mask, h, w, c, op, level):
        """marker (overwritten: one of the two ping-pong buffers), mask: keys -> (the limit, sweeps launched).  A value
        moves at least one pixel per sweep and no geodesic path is longer than h * w pixels; one more sweep for the clamp
        of a marker that lies beyond its mask, one more group to see the `changed` word stay clear."""
        be = self._backend()
        buffers = [marker, be.empty(h * w * c, torch.int32)]
        at, sweeps = 0, 0
        for _ in range(-(-(h * w + 1) // SWEEP_GROUP) + 1):
            changed = be.zeros(1, torch.int32)
            for _ in range(SWEEP_GROUP):
                be.call("morph_reconstruct_sweep_u32", Ref(buffers[at]), Ref(mask), h, w, c, op, Ref(buffers[1 - at]),
                        Ref(changed))
                at, sweeps = 1 - at, sweeps + 1
            if int(changed.cpu()[0]) == 0:
                return buffers[at], sweeps
        raise RuntimeError(f"MorphologicalProfile: level {level}: the reconstruction of a {h} x {w} raster did not settle "
                           f"in {sweeps} sweeps")

    # ------------------------------------------------------------------------------------------------ single operators
    def _radius(self, r, what):
        if isinstance(r, bool) or not isinstance(r, numbers.Integral) or not 0 <= r <= MORPH_MAX_RADIUS:
            raise ValueError(f"MorphologicalProfile.{what}: radius {r!r}: an integer in 0 .. {MORPH_MAX_RADIUS} "
                             f"(HYPEL_MORPH_MAX_RADIUS)")
        return int(r)

    def _operator(self, image, r, what, ops, reconstruct_op=None):
        r = self._radius(r, what)
        view = self._view(image, what)
        _, h, w, c, _, _ = view
        keys = result = self._keys(view)
        for op in ops:
            result = self._erode_dilate(result, h, w, c, r, op)
        if reconstruct_op is not None:
            result, _ = self._reconstruct(result, keys, h, w, c, reconstruct_op, f"{what} r={r}")
        return self._floats(result, h, w, c, image, image.ndim == 2)

    def erode(self, image, r):
        """[h, w] or [h, w, c] -> the same shape: the per-channel minimum over the element of radius r (0: a copy)"""
        return self._operator(image, r, "erode", (MORPH_ERODE,))

    def dilate(self, image, r):
        return self._operator(image, r, "dilate", (MORPH_DILATE,))

    def opening(self, image, r):
        """by reconstruction (or plain, by_reconstruction=False) with this object's shape"""
        if self.by_reconstruction:
            return self._operator(image, r, "opening", (MORPH_ERODE,), MORPH_DILATE)
        return self._operator(image, r, "opening", (MORPH_ERODE, MORPH_DILATE))

    def closing(self, image, r):
        if self.by_reconstruction:
            return self._operator(image, r, "closing", (MORPH_DILATE,), MORPH_ERODE)
        return self._operator(image, r, "closing", (MORPH_DILATE, MORPH_ERODE))

    def reconstruct(self, marker, mask, method="dilation"):
        """The limit of m <- min(dilate3x3(m), mask) from min(marker, mask) (method "erosion": the dual), 8-connectivity."""
        if method not in METHODS:
            raise ValueError(f"MorphologicalProfile.reconstruct: method={method!r}: one of {tuple(METHODS)}")
        marker_view, mask_view = self._view(marker, "reconstruct"), self._view(mask, "reconstruct")
        _, h, w, c, _, _ = mask_view
        if marker_view[1:4] != (h, w, c):
            raise ValueError(f"MorphologicalProfile.reconstruct: a marker of shape {tuple(marker.shape)} for a mask of "
                             f"shape {tuple(mask.shape)}")
        result, _ = self._reconstruct(self._keys(marker_view), self._keys(mask_view), h, w, c, METHODS[method],
                                      f"reconstruct by {method}")
        return self._floats(result, h, w, c, mask, mask.ndim == 2)

    # ------------------------------------------------------------------------------------------------ profiles
    def _profile(self, name, view, pad, out, out_c, first_base):
        """the profiles of the c channels of `view` into channels first_base (2 S + 1) ... of the padded stack `out`"""
        _, h, w, c, _, _ = view
        levels = len(self.radii)
        step = 2 * levels + 1
        base = self._keys(view)
        self._store(base, h, w, c, pad, out, out_c, first_base * step + levels, step)
        for i, r in enumerate(self.radii, 1):
            for kind, first, second, channel in (("opening", MORPH_ERODE, MORPH_DILATE, levels + i),
                                                 ("closing", MORPH_DILATE, MORPH_ERODE, levels - i)):
                level = self._erode_dilate(base, h, w, c, r, first)
                if self.by_reconstruction:
                    level, self.sweeps_[f"{name}/{kind}/{r}"] = self._reconstruct(level, base, h, w, c, second,
                                                                                  f"{name}/{kind}/{r}")
                else:
                    level = self._erode_dilate(level, h, w, c, r, second)
                self._store(level, h, w, c, pad, out, out_c, first_base * step + channel, step)

    def transform(self, image):
        """[h, w, c] (or [h, w]) -> [h, w, c (2 S + 1)].  A NumPy array comes back as one, a device tensor as one."""
        view = self._view(image, "transform")
        _, h, w, c, _, _ = view
        out_c = c * (2 * len(self.radii) + 1)
        out = self._backend().empty(h * w * out_c)
        self.sweeps_ = {}
        self._profile("image", view, 0, out, out_c, 0)
        out = out.view(h, w, out_c)
        return out.cpu().numpy() if isinstance(image, np.ndarray) else out

    def transform_scene(self, data_set):
        """The profile of the INTERIOR of the data set's padded rasters (the padding rows are reflections and would act
        as structure that is not there), written back with the same symmetric padding.  -> ProjectedScene"""
        if getattr(data_set, "_data_sets", None) is not None:
            raise NotImplementedError("MorphologicalProfile.transform_scene: a MultiDataSet (GULFPORTALT) draws every sample "
                                      "from one of several scenes; a profile of several scenes at once is not built "
                                      "(DESIGN 7)")
        if int(getattr(data_set, "casi_scale", 1)) != 1:
            raise NotImplementedError("MorphologicalProfile.transform_scene: a two-resolution scene (casi_scale == 2, "
                                      "GRSS2018): a radius means different ground distances on the two grids and the "
                                      "LiDAR bases cannot join the HSI stack; not built (DESIGN 7)")
        from hypelcnn_amd.common.common_nn_ops import SceneArrays
        be = self._backend()
        casi, lidar = SceneArrays._resident(data_set, be.device)
        pad = int(data_set.neighborhood)
        hp, wp = int(casi.shape[0]), int(casi.shape[1])
        h, w = hp - 2 * pad, wp - 2 * pad
        if pad > min(h, w):
            raise ValueError(f"MorphologicalProfile.transform_scene: a padding of {pad} around a {h} x {w} interior")
        rasters = [("hsi", casi)]
        if self.include_lidar and lidar is not None:
            rasters.append(("lidar", lidar))
        step = 2 * len(self.radii) + 1
        out_c = sum(int(r.shape[2]) for _, r in rasters) * step
        out = be.empty(hp * wp * out_c)
        self.sweeps_ = {}
        first_base = 0
        for name, raster in rasters:
            self._profile(name, self._view(raster[pad:hp - pad, pad:wp - pad, :], "transform_scene"), pad, out, out_c,
                          first_base)
            first_base += int(raster.shape[2])
        return ProjectedScene(data_set, out.view(hp, wp, out_c), None if self.include_lidar else lidar)
