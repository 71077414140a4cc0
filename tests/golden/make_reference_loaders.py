#!/usr/bin/env python3
"""Pin the four file-backed loaders by executing the reference's own text (build container only; needs
/root/reference).

`loader/GRSS2013DataLoader.py`, `GULFPORTDataLoader.py`, `GULFPORTALTDataLoader.py` and `AVONDataLoader.py` run
UNCHANGED on the seeded data directory of tests/loader_cases.py; `tifffile` / `imageio.v2` are stand-ins that delegate
to the project's tiff_io / bmp_io, `tensorflow` and `tensorflow_gan` are the usual stand-ins (the loaders only build
lazy shadow-augmenter structs from them).

Written to tests/golden/reference_loaders.json / .npz -- digests, not scenes: per case the extrema, the AVON clip
bounds, the shadow ratio, scene and data shapes, the rows of read_targets in order, the patches at loader_cases.POINTS,
the float64 sum of the prepared scene; per loader the colour list and band measurements.  Only data is written."""
import importlib
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import tf_standin as S  # noqa: E402
from tests import loader_cases as C  # noqa: E402


def digest(arrays, meta, key, data_set, members=None):
    prim = data_set if members is None else members[0]
    for name in ("casi_min", "casi_max", "lidar_min", "lidar_max"):
        arrays[f"{key}/{name}"] = np.asarray(getattr(prim, name))
    arrays[f"{key}/patches"] = np.stack([np.asarray(prim.get_data_point(x, y)) for x, y in C.POINTS])
    arrays[f"{key}/scene_sum"] = np.asarray(
        [np.sum(np.asarray(prim.casi, np.float32), dtype=np.float64),
         0.0 if prim.lidar is None else np.sum(np.asarray(prim.lidar, np.float32), dtype=np.float64)])
    meta[key] = {"scene_shape": [int(v) for v in data_set.get_scene_shape()],
                 "data_shape": [int(v) for v in data_set.get_data_shape()],
                 "casi_dtype": str(data_set.get_unnormalized_casi_dtype()),
                 "creators": sorted(data_set.shadow_creator_dict) if data_set.shadow_creator_dict else None}
    if members is not None:
        for i, m in enumerate(members):
            arrays[f"{key}/member{i}/patches"] = np.stack([np.asarray(m.get_data_point(x, y)) for x, y in C.POINTS])
        meta[key]["members"] = [next(j for j, d in enumerate(members) if d is m) for m in members]


def main():
    S.install()
    import tfgan_standin as TG
    TG.install()
    from hypelcnn_amd.common import bmp_io, tiff_io
    sys.modules["tifffile"] = types.SimpleNamespace(imread=tiff_io.imread, imwrite=tiff_io.imwrite)
    imageio = types.ModuleType("imageio")
    imageio.v2 = types.ModuleType("imageio.v2")
    imageio.v2.imread = bmp_io.imread
    sys.modules["imageio"], sys.modules["imageio.v2"] = imageio, imageio.v2
    ref_loader = importlib.import_module("loader.DataLoader")
    base = C.write_data_dir(tempfile.mkdtemp())
    meta, arrays = {"neighborhood": C.NEIGHBORHOOD, "points": C.POINTS, "loaders": {}}, {}
    nb = C.NEIGHBORHOOD
    for name in C.LOADERS:
        cls = getattr(importlib.import_module("loader." + name), name)
        loader = cls(base)
        meta["loaders"][name] = {"model_base_dir": loader.get_model_base_dir()[len(base):],
                                 "class_count": [loader.get_class_count().start, loader.get_class_count().stop]}
        arrays[f"{name}/colors"] = np.asarray(loader.get_samples_color_list())
        arrays[f"{name}/bands"] = np.asarray(loader.get_band_measurements())
        cases = [("normalized", {}, True), ("raw", {}, False)]
        if name == "AVONDataLoader":
            cases.append(("shcorrected", {"load_shadow_corrected": True}, True))
        if name == "GULFPORTALTDataLoader":
            cases = [(m.name.lower(), {"_load_mode": m}, True) for m in ref_loader.LoadingMode]
        for case, attrs, normalize in cases:
            for k, v in attrs.items():
                setattr(loader, k, v)
            data_set = loader.load_data(nb, normalize)
            key = f"{name}/{case}"
            members = getattr(data_set, "_data_sets", None)
            digest(arrays, meta, key, data_set, members)
            shadow = loader.load_shadow_map(nb, data_set)
            if shadow is None:
                meta[key]["shadow_map"] = None
            else:
                arrays[f"{key}/shadow_map_sum"] = np.asarray(int(np.asarray(shadow[0], np.int64).sum()))
                arrays[f"{key}/shadow_ratio"] = np.asarray(shadow[1])
            if name == "AVONDataLoader" and case == "normalized":
                tif = importlib.import_module("tifffile")
                raw = np.swapaxes(tif.imread(loader.get_model_base_dir() + "0920-1857.georef_cropped.tif")
                                  [:, :, C.BLANK:-C.BLANK], 0, 2).astype(np.uint16)
                arrays[f"{key}/clip_bounds"] = np.percentile(raw, 95, axis=[0, 1]).astype(np.uint16)
            for k in attrs:
                setattr(loader, k, {"load_shadow_corrected": False, "_load_mode": ref_loader.LoadingMode.ORIGINAL}[k])
        # target rows that involve no random draw
        if name == "GRSS2013DataLoader":
            arrays[f"{name}/targets/TR"] = loader.read_targets("2013_IEEE_GRSS_DF_Contest_Samples_TR.tif")
            arrays[f"{name}/targets/VA"] = loader.read_targets("2013_IEEE_GRSS_DF_Contest_Samples_VA.tif")
            s = loader.load_samples(1.0, 0)
            arrays[f"{name}/samples_ratio0/training"], arrays[f"{name}/samples_ratio0/validation"] = \
                s.training_targets, s.validation_targets
        elif name in ("GULFPORTDataLoader", "GULFPORTALTDataLoader"):
            arrays[f"{name}/targets/gt"] = loader.read_targets("muulf_gt.tif")
            arrays[f"{name}/targets/gt_shadow_corrected"] = loader.read_targets("muulf_gt_shadow_corrected.tif")
        else:
            for no in (1, 2):
                for kind in ("nsh", "sh"):
                    arrays[f"{name}/targets/{no}_{kind}"] = loader.read_each_target(
                        f"0920-1857.georef_cropped_rgb_with_targets_{no}_{kind}.bmp", target_no=no)
        np.random.seed(5)
        s = loader.load_samples(0.7 if name != "GRSS2013DataLoader" else 1.0, 0.2 if name != "GULFPORTALTDataLoader" else 0)
        meta["loaders"][name]["split_sizes"] = {part: np.bincount(np.asarray(getattr(s, part + "_targets"))[:, 2].astype(int),
                                                                 minlength=loader.get_class_count().stop).tolist()
                                               for part in ("training", "test", "validation")}
    shutil.rmtree(base)
    with open(os.path.join(HERE, "reference_loaders.json"), "w") as f:
        json.dump(meta, f, sort_keys=True, indent=0, separators=(",", ":"))
    np.savez_compressed(os.path.join(HERE, "reference_loaders.npz"), **arrays)
    print("wrote reference_loaders.json / .npz:", len(arrays), "arrays")


if __name__ == "__main__":
    main()
