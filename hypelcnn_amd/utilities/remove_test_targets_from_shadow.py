"""Take the validation targets out of a scene's shadow map (reference utilities/remove_test_targets_from_shadow.py), so
that a shadow GAN trained against the map never sees a pixel the classifier is scored on:

    python -m hypelcnn_amd.utilities.remove_test_targets_from_shadow --loader_name GRSS2013DataLoader --path <dir> \
        --output_path <dir>

Reads the loader's shadow map, clears it at every validation target that lies in shadow and writes `shadow_map.tif`
(the file GRSS2013DataLoader.load_shadow_map reads) under --output_path.  A few thousand host lookups: no launch."""
import argparse
import os

import numpy

from hypelcnn_amd.common.cmd_parser import add_parse_cmds_for_loaders, add_parse_cmds_for_loggers
from hypelcnn_amd.common.common_nn_ops import get_loader_from_name
from hypelcnn_amd.common.tiff_io import imwrite


def build_parser():
    parser = argparse.ArgumentParser()
    add_parse_cmds_for_loggers(parser)
    add_parse_cmds_for_loaders(parser)
    return parser


def main(argv=None, backend=None):
    """-> {"cleared": validation targets that were in shadow, "non_shadow": those that were not}."""
    flags, _ = build_parser().parse_known_args(argv)
    loader = get_loader_from_name(flags.loader_name, flags.path)
    if backend is not None and hasattr(loader, "backend"):
        loader.backend = backend
    sample_set = loader.load_samples(0.1, 0.1)
    shadow_map, _ = loader.load_shadow_map(0, None)
    shadow_map = numpy.array(shadow_map, copy=True)
    cleared = non_shadow = 0
    for point in numpy.asarray(sample_set.validation_targets).astype(int):
        if shadow_map[point[1], point[0]] == 1:
            shadow_map[point[1], point[0]] = 0
            cleared += 1
        else:
            non_shadow += 1
    os.makedirs(flags.output_path, exist_ok=True)
    imwrite(os.path.join(flags.output_path, "shadow_map.tif"), shadow_map)
    return {"cleared": cleared, "non_shadow": non_shadow}


if __name__ == "__main__":
    main()
