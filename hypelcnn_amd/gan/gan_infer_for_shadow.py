"""Checkpoint scoring with the band-ratio JS-divergence statistic (reference gan/gan_infer_for_shadow.py:12-55), same
flags.

    python -m hypelcnn_amd.gan.gan_infer_for_shadow --loader_name SyntheticDataLoader --path grss2013 \
        --gan_type cycle_gan --base_log_path <log dir>/model.ckpt-1000.npz --number_of_samples 6000

Restores the generator(s), runs the wrapper's inference hook once at iteration 0 and returns its divergences.  The
hook writes best_ratio_<suffix>.json (and a summaries.jsonl line) into the directory the reference's summary writer
uses: --base_log_path itself, without the .npz suffix; with --band_ratio_stats true also the band-ratio figure and its
numbers, band_ratio_<suffix>_0.pdf / .json."""
import argparse
import os

import numpy

from hypelcnn_amd.common.cmd_parser import add_parse_cmds_for_loaders, add_parse_cmds_for_loggers, \
    type_ensure_strtobool
from hypelcnn_amd.common.common_nn_ops import get_loader_from_name
from hypelcnn_amd.gan.gan_utilities import load_gan_variables
from hypelcnn_amd.gan.wrapper_registry import get_infer_wrapper_dict
from hypelcnn_amd.gan.wrappers import gan_common as C


def add_parse_cmds_for_app(parser):
    parser.add_argument("--number_of_samples", nargs="?", type=int, default=6000, help="Number of samples.")
    parser.add_argument("--gan_type", nargs="?", type=str, default="cycle_gan",
                        help="Gan type to train, possible values; cycle_gan, gan_x2y and gan_y2x")
    parser.add_argument("--band_ratio_stats", nargs="?", type=type_ensure_strtobool, default=False,
                        help="Write band_ratio_<suffix>_<iteration>.json / .pdf (the band-ratio figure) to the log dir.")


def build_parser():
    parser = argparse.ArgumentParser()
    add_parse_cmds_for_loaders(parser)
    add_parse_cmds_for_loggers(parser)
    add_parse_cmds_for_app(parser)
    return parser


def log_dir_of(base_log_path):
    return base_log_path[:-len(".npz")] if base_log_path.endswith(".npz") else base_log_path


def main(argv=None, backend=None):
    """-> the hook's mean divergences ([shadowed, deshadowed] for two-generator GANs, [one] otherwise)."""
    flags, _ = build_parser().parse_known_args(argv)
    if flags.neighborhood != 0:
        raise ValueError(f"gan_infer_for_shadow scores single pixels only (--neighborhood 0, got {flags.neighborhood}): "
                         f"the statistic squeezes the patch axes, which the reference cannot do for larger patches either")
    numpy.set_printoptions(precision=5, suppress=True)
    loader = get_loader_from_name(flags.loader_name, flags.path)
    data_set = loader.load_data(flags.neighborhood, True)
    shadow_map, shadow_ratio = loader.load_shadow_map(flags.neighborhood, data_set)
    wrapper = get_infer_wrapper_dict()[flags.gan_type]
    log_dir = log_dir_of(flags.base_log_path)
    os.makedirs(log_dir, exist_ok=True)
    hook = wrapper.create_inference_hook(data_set=data_set, loader=loader, log_dir=log_dir,
                                         neighborhood=flags.neighborhood, shadow_map=shadow_map,
                                         shadow_ratio=shadow_ratio, validation_iteration_count=0,
                                         validation_sample_count=flags.number_of_samples, backend=backend)
    hook.band_ratio_stats = bool(flags.band_ratio_stats)
    sess = C.restore_generators(hook.ctx, wrapper.create_generator_restorer(), load_gan_variables(flags.base_log_path))
    hook.after_create_session(sess, None)
    hook.after_run(0)
    divergences = hook.last_divergences()
    print("Output divergence values:", divergences)
    return divergences


if __name__ == "__main__":
    main()
