"""What lies under the building shadows of a labelled scene (reference utilities/reveal_shadow_targets.py):

    python -m hypelcnn_amd.utilities.reveal_shadow_targets --loader_name GULFPORTDataLoader --path <dir> \
        --output_path <dir>

The pixels labelled `--shadow_class` form the shadow map.  Every 8-connected region of it takes the class most of the
pixels around it carry -- shadow, `--building_class` and unlabelled pixels have no say, a tie goes to the smaller class,
a region with no such neighbour stays shadow -- and the un-normalised scene under the map is scaled by the lit / shadow
band ratio.  Labelling, votes, relabelling and the correction run on the device (common/device_components.py); DESIGN
§3.11 lists where this departs from the reference's walk along OpenCV's contours.  Writes, under --output_path,

    muulf_shadow_map.tif             uint8 0 / 1            (GULFPORTALTDataLoader.load_shadow_map reads it)
    muulf_hsi_shadow_corrected.tif   float32, chunky
    muulf_gt_shadow_corrected.tif    uint8, classes + 1, 255 kept   (GULFPORTALTDataLoader.load_samples reads it)
    targets.tif, targets_shadow_corrected.tif   the two figures of the reference as RGB rasters"""
import argparse
import os

import numpy
import torch

from hypelcnn_amd.common import device_components as dc
from hypelcnn_amd.common.cmd_parser import add_parse_cmds_for_loaders, add_parse_cmds_for_loggers
from hypelcnn_amd.common.common_nn_ops import create_colored_image, create_target_image_via_samples, \
    get_loader_from_name
from hypelcnn_amd.common.device_scene import device_shadow_ratio
from hypelcnn_amd.common.tiff_io import DeviceRaster, imwrite

BUILDING_CLASS = 7
BUILDING_SHADOW_CLASS = 6


def build_parser():
    parser = argparse.ArgumentParser()
    add_parse_cmds_for_loggers(parser)
    add_parse_cmds_for_loaders(parser)
    parser.add_argument("--shadow_class", nargs="?", type=int, default=BUILDING_SHADOW_CLASS,
                        help="Label (0-based) of the building-shadow class")
    parser.add_argument("--building_class", nargs="?", type=int, default=BUILDING_CLASS,
                        help="Label (0-based) of the building class, which never wins a shadow region")
    return parser


def main(argv=None, backend=None):
    """-> {"ratio": float32 [bands], "components": n, "winners": uint8 [n] (255: no proper neighbour),
    "sizes": int32 [n]}, the regions in row-major order of their first pixel."""
    flags, _ = build_parser().parse_known_args(argv)
    loader = get_loader_from_name(flags.loader_name, flags.path)
    if backend is not None and hasattr(loader, "backend"):
        loader.backend = backend
    sample_set = loader.load_samples(0.1, 0.1)
    data_set = loader.load_data(0, False)
    if backend is None:
        backend = getattr(data_set, "backend", None)
    if backend is None or getattr(data_set, "casi_dev", None) is None:
        from hypelcnn_amd.backend import HypelError
        raise HypelError("reveal_shadow_targets runs on the compute device: no HIP device is visible and the loader "
                         "prepared its scene on the host (there is no CPU fallback)")
    h, w = data_set.get_scene_shape()
    n_classes = len(loader.get_class_count())
    targets = create_target_image_via_samples(sample_set, [h, w])
    shadow_map = (targets == flags.shadow_class).astype(numpy.uint8)

    ratio = device_shadow_ratio(data_set, shadow_map)
    targets_d, map_d = backend.upload(targets), backend.upload(shadow_map)
    bands = int(data_set.casi_dev.shape[2])
    scene = DeviceRaster(data_set.casi_dev.reshape(-1).view(torch.uint8), 0, numpy.float32, (h, w, bands))
    corrected = dc.shadow_correct(backend, scene, map_d, ratio)

    root = dc.label_components(backend, map_d, h, w)
    comp, n = dc.compact_components(backend, root, h, w)
    _, size, winner = dc.component_votes(backend, targets_d, comp, h, w, n, n_classes,
                                         exclude=(flags.shadow_class, flags.building_class))
    stored = dc.relabel_components(backend, targets_d, comp, winner, h, w, plus_one=True).cpu().numpy().reshape(h, w)
    revealed = numpy.where(stored == 255, stored, stored - 1).astype(numpy.uint8)  # the figure shows plain classes

    winners, sizes = winner.cpu().numpy(), size.cpu().numpy()
    for target in winners:
        if target == 255:
            print("found contour with no proper neighbors")
        else:
            print(f"shadow converted to neighboring target {int(target):d}")

    os.makedirs(flags.output_path, exist_ok=True)
    colors = loader.get_samples_color_list()
    imwrite(os.path.join(flags.output_path, "muulf_shadow_map.tif"), shadow_map)
    imwrite(os.path.join(flags.output_path, "muulf_hsi_shadow_corrected.tif"),
            corrected.cpu().numpy().reshape(h, w, bands))
    imwrite(os.path.join(flags.output_path, "muulf_gt_shadow_corrected.tif"), stored)
    imwrite(os.path.join(flags.output_path, "targets.tif"), create_colored_image(targets, colors))
    imwrite(os.path.join(flags.output_path, "targets_shadow_corrected.tif"),
            create_colored_image(revealed, colors))
    return {"ratio": ratio, "components": n, "winners": winners, "sizes": sizes}


if __name__ == "__main__":
    main()
