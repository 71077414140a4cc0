"""The band ratio a scene's own shadowed and lit pairs have -- the target the shadow generators are trained towards
(reference utilities/measure_targets_shadow_ratio.py):

    python -m hypelcnn_amd.utilities.measure_targets_shadow_ratio --loader_name GRSS2013DataLoader --path <dir> \
        --pairing_method neighbour --output_path <dir>

Loads the scene (neighbourhood 0, normalised) and its shadow map, pairs shadowed and lit pixels with the chosen sampler
-- on the device when the scene is resident there, else on the host with one upload of the pairs -- and takes the
statistics of shadow / normal over the pairs that are finite in every band (common/band_ratio.py).  Writes
<loader>_<pairing>_0.json with the numbers and <loader>_<pairing>_0.pdf with the figure: the mean as the centre,
mean -/+ std as the band."""
import argparse

from hypelcnn_amd.common.band_ratio import band_ratio_stats, write_band_ratio
from hypelcnn_amd.common.cmd_parser import add_parse_cmds_for_loaders, add_parse_cmds_for_loggers
from hypelcnn_amd.common.common_nn_ops import get_loader_from_name
from hypelcnn_amd.gan.gan_train_for_shadow import read_hsi_data
from hypelcnn_amd.gan.wrapper_registry import get_sampling_map


def build_parser():
    parser = argparse.ArgumentParser()
    add_parse_cmds_for_loggers(parser)
    add_parse_cmds_for_loaders(parser)
    parser.add_argument("--pairing_method", nargs="?", type=str, default="random",
                        help="Pairing method for the shadowed and non-shadowed samples. "
                             "Opts: random, target, dummy, neighbour")
    return parser


def main(argv=None, backend=None):
    """-> the statistics dict of band_ratio_stats (samples, kept, p10, p50, p90, mean, std)."""
    flags, _ = build_parser().parse_known_args(argv)
    neighborhood = 0
    loader = get_loader_from_name(flags.loader_name, flags.path)
    if backend is not None and hasattr(loader, "backend"):
        loader.backend = backend
    data_set = loader.load_data(neighborhood, True)
    shadow_map, _ = loader.load_shadow_map(neighborhood, data_set)
    if backend is None:
        backend = getattr(data_set, "backend", None)
    if backend is None:
        from hypelcnn_amd.backend import HipBackend
        backend = HipBackend()
    normal, shadow = read_hsi_data(loader, data_set, shadow_map, flags.pairing_method, get_sampling_map(), backend)
    n = normal.shape[0]
    stats = band_ratio_stats(backend, shadow.reshape(n, -1), normal.reshape(n, -1), None)
    write_band_ratio(flags.output_path, f"{flags.loader_name.lower()}_{flags.pairing_method.lower()}", 0,
                     loader.get_band_measurements(), stats, stats["mean"], stats["mean"] - stats["std"],
                     stats["mean"] + stats["std"])
    return stats


if __name__ == "__main__":
    main()
