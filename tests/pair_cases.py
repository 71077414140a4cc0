"""TEST INFRASTRUCTURE: the small seeded scenes, shadow maps, target lists and sampler settings that the pair-sampling
tests and tests/golden/make_reference_pair_sampling.py share -- one builder, so that a test regenerates the inputs of
the committed fixture without the reference.

A scene is already "prepared": float32 casi [h + 2 nb, w + 2 nb, bands] (and lidar [.., 1]) as a data set holds them
after padding and normalisation; the shadow map and the targets are in scene coordinates [h, w]."""
import numpy as np

# name -> (h, w, bands, lidar, neighborhood, classes, seed)
SCENES = {
    "a": (19, 27, 6, 1, 0, 4, 101),   # the GAN trainer's geometry: 1 x 1 spectra, LiDAR present
    "b": (30, 41, 4, 0, 0, 3, 202),   # large enough for the registry's ring (20, 2); no LiDAR
    "c": (12, 15, 3, 1, 1, 3, 303),   # 3 x 3 patches
}
# case -> (scene, sampler class name, constructor arguments)
CASES = {
    "neighbour_a": ("a", "NeighborhoodBasedSampler", {"neighborhood_size": 5, "margin": 2}),
    "neighbour_registry": ("b", "NeighborhoodBasedSampler", {"neighborhood_size": 20, "margin": 2}),
    "neighbour_patches": ("c", "NeighborhoodBasedSampler", {"neighborhood_size": 3, "margin": 1}),
    "random_multiplied": ("a", "RandomBasedSampler", {"multiply_shadowed_data": True}),
    "random_plain": ("b", "RandomBasedSampler", {"multiply_shadowed_data": False}),
    "random_patches": ("c", "RandomBasedSampler", {"multiply_shadowed_data": True}),
    "target_a": ("a", "TargetBasedSampler", {"margin": 2}),
    "target_patches": ("c", "TargetBasedSampler", {"margin": 1}),
}


def shadow_map(h, w, rng):
    """uint8 [h, w] of 0 / 1: a block (about an eighth of the scene) plus 2 % single pixels; corners stay lit"""
    smap = np.zeros((h, w), np.uint8)
    smap[h // 4: h // 4 + max(2, h // 3), w // 3: w // 3 + max(2, w // 3)] = 1
    smap[rng.random((h, w)) < 0.02] = 1
    smap[0, 0] = smap[-1, -1] = 0
    return smap


def build_scene(name):
    h, w, bands, lidar, nb, classes, seed = SCENES[name]
    rng = np.random.default_rng(seed)
    casi = rng.random((h + 2 * nb, w + 2 * nb, bands)).astype(np.float32)
    lid = rng.random((h + 2 * nb, w + 2 * nb, 1)).astype(np.float32) if lidar else None
    smap = shadow_map(h, w, rng)
    # targets (x, y, class) in shuffled order over 60 % of the pixels: every class meets both sides of the map
    pick = rng.permutation(h * w)[: int(h * w * 0.6)]
    targets = np.stack([pick % w, pick // w, np.arange(pick.size) % classes], axis=1).astype(int)
    return {"casi": casi, "lidar": lid, "map": smap, "targets": targets, "neighborhood": nb, "classes": classes,
            "h": h, "w": w}


class StubDataSet:
    """What a sampler asks of a data set, over prepared arrays (BasicDataSet's accessors, common_nn_ops.py:74-89)."""

    def __init__(self, casi, lidar, neighborhood):
        self.casi, self.lidar, self.neighborhood = casi, lidar, int(neighborhood)

    def get_data_shape(self):
        side = 2 * self.neighborhood + 1
        return [side, side, self.casi.shape[2] + (0 if self.lidar is None else 1)]

    def get_casi_band_count(self):
        return self.casi.shape[2]

    def get_scene_shape(self):
        return [self.casi.shape[0] - 2 * self.neighborhood, self.casi.shape[1] - 2 * self.neighborhood]

    def get_data_point(self, point_x, point_y):
        side = 2 * self.neighborhood + 1
        win = (slice(point_y, point_y + side), slice(point_x, point_x + side))
        if self.lidar is None:
            return self.casi[win]
        return np.concatenate((self.casi[win], self.lidar[win]), axis=2)


class StubLoader:
    def __init__(self, targets, classes):
        self._targets, self._classes = targets, classes

    def read_targets(self, target_image_path):
        return self._targets.copy()

    def get_class_count(self):
        return range(0, self._classes)


def stubs(scene):
    return StubDataSet(scene["casi"], scene["lidar"], scene["neighborhood"]), StubLoader(scene["targets"], scene["classes"])
