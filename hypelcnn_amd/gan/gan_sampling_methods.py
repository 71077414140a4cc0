"""Pairing of shadowed / non-shadowed pixels for GAN training (reference gan/gan_sampling_methods.py:16-201).

`get_sample_pairs` is the host path: vectorised numpy restatements (the reference walks the scene with Python double
loops); pixel order is the reference's row-major scan order, so results are identical
(tests/test_pair_sampling_emu.py checks them against pairs the reference's own samplers produced).

`get_sample_pairs_device` is the same pairing for a scene that lives on the compute device (common/device_scene.py):
the shadow map is uploaded, csrc/pairs.hip turns it into the two point lists -- dilations, selection masks, ordered
compaction, repeat / remainder expansion -- and hypel_gather_patches_f32 cuts the pairs from the resident scene.  The
scene is never downloaded and the pairs are the host path's, bit for bit."""
from abc import ABC, abstractmethod

import numpy
import torch
from scipy import ndimage

from hypelcnn_amd.backend import COMPACT_TILE, Ref


class Sampler(ABC):
    @abstractmethod
    def get_sample_pairs(self, data_set, loader, shadow_map):
        pass


def _gather(data_set, mask):
    """Patches of all pixels where mask == 1, row-major (x_index outer = rows, y_index inner = columns)."""
    rows, cols = numpy.nonzero(mask == 1)
    shape = data_set.get_data_shape()
    out = numpy.zeros([len(rows)] + list(shape), dtype=numpy.float32)
    for i, (r, c) in enumerate(zip(rows, cols)):
        out[i] = data_set.get_data_point(c, r)
    return out


# ----------------------------------------------------------------------------- device path (csrc/pairs.hip)
def _device_map(data_set, shadow_map):
    """The shadow map as the uint8 [h, w] raster the launches read.  Refused: a map that is not the scene's size (the
    gather does not clip its windows) or that holds anything but 0 and 1 (the reference tells shadow by == 1 in its
    loops and by != 0 in its dilations: the two only agree on a 0 / 1 map)."""
    smap = numpy.asarray(shadow_map)
    h, w = (int(v) for v in data_set.get_scene_shape())
    if smap.ndim != 2 or smap.shape != (h, w):
        raise ValueError(f"device pairing: shadow map {smap.shape} is not the scene's {(h, w)}")
    if not numpy.isin(smap, (0, 1)).all():
        raise ValueError("device pairing: the shadow map has values other than 0 and 1")
    return numpy.ascontiguousarray(smap, dtype=numpy.uint8)


def device_dilate(backend, map_d, h, w, radius):
    """binary_dilation(map, iterations=radius) of a uint8 device raster: uint8 device tensor [h * w]"""
    out = backend.empty(h * w, torch.uint8)
    ws = backend.empty(h * w, torch.int32)
    backend.call("mask_dilate_l1_u8", Ref(map_d), h, w, int(radius), Ref(out), Ref(ws))
    return out


def device_pair_masks(backend, map_d, n, reach=None, margin=None):
    shadow, lit = backend.empty(n, torch.uint8), backend.empty(n, torch.uint8)
    backend.call("pair_masks_u8", Ref(map_d), None if reach is None else Ref(reach),
                 None if margin is None else Ref(margin), n, Ref(shadow), Ref(lit))
    return shadow, lit


def device_compact(backend, mask_d, h, w):
    """(x, y) of the set pixels of a uint8 device raster in row-major order: int32 device tensor [n, 2].  The count
    comes back to the host (four bytes): it sizes everything after it."""
    n = h * w
    points = backend.empty(2 * n, torch.int32)
    count = backend.empty(1, torch.int32)
    ws = backend.empty((n + COMPACT_TILE - 1) // COMPACT_TILE, torch.int32)
    backend.call("mask_compact_points_i32", Ref(mask_d), h, w, Ref(points), n, Ref(count), Ref(ws))
    found = int(count.cpu()[0])
    return points[:2 * found].reshape(found, 2)


def device_expand(backend, points, repeat, remainder=0):
    """numpy.vstack([numpy.repeat(points, repeat, axis=0), points[0:remainder]]) of an int32 [n, 2] device tensor"""
    n = int(points.shape[0])
    out = backend.empty(2 * (n * repeat + remainder), torch.int32)
    backend.call("points_expand_i32", Ref(points.reshape(-1)), n, int(repeat), int(remainder), Ref(out))
    return out.reshape(-1, 2)


def device_gather(backend, data_set, points, hsi_only=False):
    """get_data_point at every row of `points` (int32 [n, 2] device tensor, scene coordinates): float32 device tensor
    [n, p, p, C], C = the casi bands alone with hsi_only.  A scene already on the device is read where it is."""
    from hypelcnn_amd.common.common_nn_ops import SceneArrays
    casi, lidar = SceneArrays._resident(data_set, backend.device)
    n, nb = int(points.shape[0]), int(data_set.neighborhood)
    p = 2 * nb + 1
    hp, wp, cc = (int(v) for v in casi.shape)
    pts = points.contiguous()
    if int(getattr(data_set, "casi_scale", 1)) == 2:
        # GRSS2018: the HSI at half the LiDAR grid's resolution; that launch always cuts both rasters
        cl = int(lidar.shape[2])
        out = torch.empty((n, p, p, cc + cl), dtype=torch.float32, device=casi.device)
        backend.call("gather_patches_2x_f32", Ref(casi.reshape(-1)), Ref(lidar.reshape(-1)), wp, int(lidar.shape[1]), cc,
                     cl, nb, Ref(pts.reshape(-1)), n, p, Ref(out.reshape(-1)))
        return out[..., :cc].contiguous() if hsi_only else out
    if hsi_only:
        lidar = None
    cl = 0 if lidar is None else int(lidar.shape[2])
    out = torch.empty((n, p, p, cc + cl), dtype=torch.float32, device=casi.device)
    backend.call("gather_patches_f32", Ref(casi.reshape(-1)), None if lidar is None else Ref(lidar.reshape(-1)), hp, wp,
                 cc, cl, Ref(pts.reshape(-1)), n, p, Ref(out.reshape(-1)))
    return out


def _both_sides(shadow_points, lit_points, lit_name):
    if shadow_points.shape[0] == 0:
        raise ValueError("device pairing: the shadow map has no shadowed pixel")
    if lit_points.shape[0] == 0:
        raise ValueError(f"device pairing: {lit_name}")


class NeighborhoodBasedSampler(Sampler):
    """Normal samples come from a ring around the shadows: dilation(neighborhood_size) minus dilation(margin)."""

    def __init__(self, neighborhood_size, margin):
        self._margin = margin
        self._neighborhood_size = neighborhood_size

    def get_sample_pairs(self, data_set, loader, shadow_map):
        ring = ndimage.binary_dilation(shadow_map, iterations=self._neighborhood_size).astype(shadow_map.dtype) - \
            ndimage.binary_dilation(shadow_map, iterations=self._margin).astype(shadow_map.dtype)
        shadow = _gather(data_set, shadow_map)
        normal = _gather(data_set, numpy.where(shadow_map == 1, 0, ring))
        return normal[0:shadow.shape[0]], shadow

    def get_sample_pairs_device(self, data_set, loader, shadow_map, backend, hsi_only=False):
        if self._margin < 1 or self._neighborhood_size < 1:
            raise ValueError(f"device pairing: margin {self._margin} and neighborhood_size {self._neighborhood_size} "
                             f"must both be at least 1 (a dilation by 0 iterations runs until nothing changes)")
        smap = _device_map(data_set, shadow_map)
        h, w = smap.shape
        map_d = backend.upload(smap)
        reach = device_dilate(backend, map_d, h, w, self._neighborhood_size)
        margin = device_dilate(backend, map_d, h, w, self._margin)
        shadow_mask, lit_mask = device_pair_masks(backend, map_d, h * w, reach, margin)
        shadow_points = device_compact(backend, shadow_mask, h, w)
        lit_points = device_compact(backend, lit_mask, h, w)
        _both_sides(shadow_points, lit_points, "no lit pixel lies in the ring around the shadows")
        lit_points = lit_points[0:shadow_points.shape[0]]
        return device_gather(backend, data_set, lit_points, hsi_only), \
            device_gather(backend, data_set, shadow_points, hsi_only)


class RandomBasedSampler(Sampler):
    def __init__(self, multiply_shadowed_data):
        self._multiply_shadowed_data = multiply_shadowed_data

    def get_sample_pairs(self, data_set, loader, shadow_map):
        shadow = _gather(data_set, shadow_map)
        normal = _gather(data_set, numpy.where(shadow_map == 1, 0, 1))
        if self._multiply_shadowed_data:
            shadow = numpy.repeat(shadow, repeats=(normal.shape[0] // shadow.shape[0]), axis=0)
        return normal[0:shadow.shape[0]], shadow

    def get_sample_pairs_device(self, data_set, loader, shadow_map, backend, hsi_only=False):
        smap = _device_map(data_set, shadow_map)
        h, w = smap.shape
        map_d = backend.upload(smap)
        shadow_mask, lit_mask = device_pair_masks(backend, map_d, h * w)
        shadow_points = device_compact(backend, shadow_mask, h, w)
        lit_points = device_compact(backend, lit_mask, h, w)
        _both_sides(shadow_points, lit_points, "the shadow map has no lit pixel")
        if self._multiply_shadowed_data:
            repeat = int(lit_points.shape[0]) // int(shadow_points.shape[0])
            if repeat == 0:
                raise ValueError("device pairing: fewer lit than shadowed pixels, repeating the shadowed ones "
                                 "0 times leaves no pair")
            shadow_points = device_expand(backend, shadow_points, repeat)
        lit_points = lit_points[0:shadow_points.shape[0]]
        return device_gather(backend, data_set, lit_points, hsi_only), \
            device_gather(backend, data_set, shadow_points, hsi_only)


class TargetBasedSampler(Sampler):
    """Pairs shadowed and lit pixels of the same class (needs the loader's class raster)."""

    def __init__(self, margin):
        self._margin = margin

    def _class_groups(self, data_set, loader, shadow_map):
        """[(rows in shadow, rows in the light)] of every class that has both, in class order; rows are (x, y, class)
        of the targets that keep the margin from the scene's border, in the target list's order."""
        targets = loader.read_targets("shadow_gen_model/class_result.tif").copy()
        h, w = data_set.get_scene_shape()
        m = self._margin
        ok = (targets[:, 1] > m) & (targets[:, 1] < h - m) & (targets[:, 0] > m) & (targets[:, 0] < w - m)
        targets[~ok, 2] = -1
        groups = []
        for cls in range(loader.get_class_count().stop):
            rows = targets[targets[:, 2] == cls]
            if not len(rows):
                continue
            in_shadow = shadow_map[rows[:, 1], rows[:, 0]] == 1
            if in_shadow.any() and not in_shadow.all():
                groups.append((rows[in_shadow], rows[~in_shadow]))
        return groups

    def get_sample_pairs(self, data_set, loader, shadow_map):
        normal_all, shadow_all = [], []
        for sh_rows, no_rows in self._class_groups(data_set, loader, shadow_map):
            sh = numpy.asarray([data_set.get_data_point(x, y) for x, y, _ in sh_rows], numpy.float32)
            no = numpy.asarray([data_set.get_data_point(x, y) for x, y, _ in no_rows], numpy.float32)
            mult, rem = len(no) // len(sh), len(no) % len(sh)
            shadow_all.append(numpy.vstack([numpy.repeat(sh, mult, axis=0), sh[0:rem]]))
            normal_all.append(no)
        return numpy.vstack(normal_all), numpy.vstack(shadow_all)

    def get_sample_pairs_device(self, data_set, loader, shadow_map, backend, hsi_only=False):
        """The target list is small and the shadow map a host array: reading, margin filter and per-class grouping
        stay host NumPy.  The device expands every class's shadowed points and cuts the patches."""
        smap = _device_map(data_set, shadow_map)
        h, w = smap.shape
        groups = self._class_groups(data_set, loader, smap)
        if not groups:
            raise ValueError("device pairing: no class has both a shadowed and a lit target")
        for rows in (r for g in groups for r in g):
            if rows[:, 0].min() < 0 or rows[:, 0].max() >= w or rows[:, 1].min() < 0 or rows[:, 1].max() >= h:
                raise ValueError("device pairing: a target lies outside the scene")
        sh_d = backend.upload(numpy.vstack([sh[:, :2] for sh, _ in groups]).astype(numpy.int32))
        no_d = backend.upload(numpy.vstack([no[:, :2] for _, no in groups]).astype(numpy.int32)).reshape(-1, 2)
        shadow_points = backend.empty(no_d.numel(), torch.int32)
        sh_at = out_at = 0
        for sh, no in groups:  # one small launch per class, into its rows of the list
            backend.call("points_expand_i32", Ref(sh_d, 2 * sh_at), len(sh), len(no) // len(sh), len(no) % len(sh),
                         Ref(shadow_points, 2 * out_at))
            sh_at += len(sh)
            out_at += len(no)
        return device_gather(backend, data_set, no_d, hsi_only), \
            device_gather(backend, data_set, shadow_points.reshape(-1, 2), hsi_only)


class DummySampler(Sampler):
    """Known-answer pair source: y == fill_value, x == fill_value * coefficient (ideal generator = x / coefficient)."""

    def __init__(self, element_count, fill_value, coefficient):
        self._element_count = element_count
        self._fill_value = fill_value
        self._coefficient = coefficient

    def get_sample_pairs(self, data_set, loader, shadow_map):
        shape = data_set.get_data_shape()
        shadow = numpy.full(numpy.concatenate([[self._element_count], shape]), fill_value=self._fill_value,
                            dtype=numpy.float32)
        return shadow * self._coefficient, shadow
