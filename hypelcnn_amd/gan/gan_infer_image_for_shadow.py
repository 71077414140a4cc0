"""Whole-scene shadow conversion with a trained generator (reference gan/gan_infer_image_for_shadow.py:15-104), same
flags.

    python -m hypelcnn_amd.gan.gan_infer_image_for_shadow --loader_name SyntheticDataLoader --path grss2013 \
        --gan_type cycle_gan --base_log_path <log dir>/model.ckpt-1000.npz --make_them_shadow shadow --output_path out/

The reference calls sess.run once per pixel.  Here the normalised scene [H*W, bands] is uploaded once and written
back as pass-through by one hypel_denorm_scatter over every pixel; the selected pixels then go through the generator
in fixed-size chunks (hypel_gather_patches_f32 with p = 1 into the phase input, one generator forward, a
hypel_denorm_scatter of the chunk into its raster rows), and the raster is copied back once.

With --rgb true the reference's second output is written too: the sRGB rendering of the converted scene (CIE 1931
2 degree observer, common/hsi_rgb_converter.py), one hypel_hsi_to_srgb launch over the raster before it leaves the
device, saved as shadow_image_rgb_{mode}_{step}_{'' | '_all'}.tif.  The flag defaults to false, which leaves the
output directory as it was before the rendering existed."""
import argparse
import os
import time

import numpy
import torch

from hypelcnn_amd.backend import OUT_DTYPES, Ref
from hypelcnn_amd.common.cmd_parser import add_parse_cmds_for_loaders, add_parse_cmds_for_loggers, \
    type_ensure_strtobool
from hypelcnn_amd.common.common_nn_ops import get_loader_from_name
from hypelcnn_amd.common.hsi_rgb_converter import render_raster_rgb
from hypelcnn_amd.common.tiff_io import imwrite
from hypelcnn_amd.gan.gan_utilities import GeneratorAugmenter, load_gan_variables
from hypelcnn_amd.gan.wrapper_registry import get_infer_wrapper_dict

MIN_BANDS = 8  # the generator's narrowest layer has bands // 8 taps (gan.hip, hypel_gan_generator_fwd)
DEFAULT_CHUNK = 65536


def add_parse_cmds_for_app(parser):
    parser.add_argument("--gan_type", nargs="?", type=str, default="cycle_gan",
                        help="Gan type to train, possible values; cycle_gan, gan_x2y and gan_y2x")
    parser.add_argument("--make_them_shadow", nargs="?", type=str, default="",
                        help="makes the scene shadowed(shadow), non shadowed(deshadow), or empty(none)")
    parser.add_argument("--convert_all", nargs="?", type=type_ensure_strtobool, default=False,
                        help="Whether to convert filtered pixels(shadowed or not) or all.")
    parser.add_argument("--rgb", nargs="?", type=type_ensure_strtobool, default=False,
                        help="Whether to write the sRGB rendering of the converted scene next to it.")


def parse_mode(make_them_shadow):
    """reference :37-47 -> (mode name, is_shadow_graph, shadow-map value to convert)"""
    if make_them_shadow == "shadow":
        return "shadow", True, 0
    if make_them_shadow == "deshadow":
        return "deshadow", False, 1
    return "none", True, -1


def select_pixels(shadow_map, mode, convert_all):
    """Row-major flat indices (y * W + x) of the pixels that go through the generator (reference :72-81)."""
    if convert_all:
        return numpy.arange(shadow_map.size, dtype=numpy.int64)
    return numpy.flatnonzero(numpy.asarray(shadow_map).reshape(-1) == parse_mode(mode)[2]).astype(numpy.int64)


def denorm_params(data_set):
    """Per-band float32 scale / offset of ((g * casi_max) + casi_min).astype(dtype): casi_max / casi_min are float32 or
    the scene's integer dtype, and NumPy promotes both to float32 against the float32 generator output."""
    dtype = numpy.dtype(data_set.get_unnormalized_casi_dtype())
    if dtype not in OUT_DTYPES:
        raise ValueError(f"scene dtype {dtype} is not supported by the shadow conversion (float32, uint16, int16, uint8): "
                         f"NumPy would evaluate the de-normalisation in float64")
    bands = data_set.get_casi_band_count()
    scale = numpy.broadcast_to(numpy.asarray(data_set.casi_max).astype(numpy.float32), (bands,))
    offset = numpy.broadcast_to(numpy.asarray(data_set.casi_min).astype(numpy.float32), (bands,))
    return dtype, numpy.ascontiguousarray(scale), numpy.ascontiguousarray(offset)


class GeneratorChunks:
    """The inference generator as fixed-size phases of one tower: `input(n)` is the phase's input buffer ([n * bands]
    float32, what the gather writes), `__call__(n)` runs the generator on it and returns the [n, bands] output (a
    strided view of the plan buffer, valid until the next call at this size).  One phase is compiled per size."""

    def __init__(self, inference_wrapper, is_shadow_graph, bands, backend):
        self.aug = GeneratorAugmenter(inference_wrapper, is_shadow_graph, bands, backend)

    def load(self, variables):
        self.aug.load(variables)

    def _phase(self, n):
        sess = self.aug.ctx.session()
        return sess.compile_phase(self.aug.tower, n, outputs=[self.aug.out], key="convert")

    def input(self, n):
        return self._phase(n).plan.buffers["in:x"]

    def __call__(self, n):
        ct = self._phase(n)
        ct.forward()
        return ct.value(self.aug.out, copy=False)


def convert_scene(data_set, shadow_map, mode, convert_all, apply_generator, backend, chunk=DEFAULT_CHUNK, timings=None,
                  rgb_band_measurements=None):
    """The converted scene [H, W, bands] in the scene's original dtype (reference :66-85).

    apply_generator: `input(n)` / `__call__(n)` as GeneratorChunks (tests plug a scripted generator in here).  The
    pass-through pixels are the normalised input put through the same de-normalisation, as in the reference.

    rgb_band_measurements: the loader's band wavelengths; when given, the finished raster is also rendered to sRGB
    while it is still on the device (reference :97-100) and (scene, uint8 [H, W, 3]) is returned."""
    h, w = data_set.get_scene_shape()
    bands = data_set.get_casi_band_count()
    if data_set.neighborhood != 0:
        raise ValueError("convert_scene: the scene must be loaded with neighborhood 0")
    dtype, scale, offset = denorm_params(data_set)
    code = OUT_DTYPES[dtype]
    rows = select_pixels(shadow_map, mode, convert_all)
    t = timings if timings is not None else {}
    t0 = time.perf_counter()
    casi = numpy.ascontiguousarray(data_set.casi[:, :, :bands], numpy.float32).reshape(h * w, bands)
    scene = backend.upload(casi)
    sc, of = backend.upload(scale), backend.upload(offset)
    raster = backend.empty(h * w * bands * dtype.itemsize, torch.uint8)
    n_sel = rows.size
    if n_sel:
        points = numpy.stack([rows % w, rows // w], axis=1).astype(numpy.int32)  # (x, y) of each selected pixel
        points_dev, rows_dev = backend.upload(points), backend.upload(rows)
    backend.synchronize()
    t["setup_s"] = time.perf_counter() - t0
    t["generator_s"] = 0.0
    t0 = time.perf_counter()
    backend.call("denorm_scatter", Ref(scene), bands, None, h * w, bands, Ref(sc), Ref(of), code, Ref(raster), bands)
    backend.synchronize()
    t["passthrough_s"] = time.perf_counter() - t0
    t["denorm_s"] = t["passthrough_s"]
    for start in range(0, n_sel, chunk):
        n = min(chunk, n_sel - start)
        t1 = time.perf_counter()
        backend.call("gather_patches_f32", Ref(scene), None, h, w, bands, 0, Ref(points_dev, 2 * start), n, 1,
                     Ref(apply_generator.input(n)))
        out = apply_generator(n)
        backend.synchronize()
        t2 = time.perf_counter()
        ld = out.stride(0)
        flat = out.as_strided(((n - 1) * ld + bands,), (1,))  # the [n, bands] rows of stride ld as one flat range
        backend.call("denorm_scatter", Ref(flat), ld, Ref(rows_dev, start), n, bands, Ref(sc), Ref(of), code,
                     Ref(raster), bands)
        backend.synchronize()
        t["generator_s"] += t2 - t1
        t["denorm_s"] += time.perf_counter() - t2
    if rgb_band_measurements is not None:
        t3 = time.perf_counter()
        rgb = render_raster_rgb(backend, raster, dtype, h, w, bands, rgb_band_measurements, offset, scale)
        t["rgb_s"] = time.perf_counter() - t3
    t3 = time.perf_counter()
    image = raster.cpu().numpy().view(dtype).reshape(h, w, bands)
    t["copy_back_s"] = time.perf_counter() - t3
    t["pixels"] = int(h * w)
    t["converted"] = int(n_sel)
    return image if rgb_band_measurements is None else (image, rgb)


def checkpoint_step(base_log_path):
    """`{step}` of the output name: what the reference takes from the TF checkpoint prefix (...model.ckpt-<step>)."""
    step = base_log_path.rsplit("-", 1)[-1]
    return step[:-len(".npz")] if step.endswith(".npz") else step


def output_name(mode, base_log_path, convert_all):
    return f"shadow_image_{mode}_{checkpoint_step(base_log_path)}{'' if not convert_all else '_all'}.tif"


def rgb_output_name(mode, base_log_path, convert_all):
    """The reference's name, stray underscore included (:101-102)."""
    return f"shadow_image_rgb_{mode}_{checkpoint_step(base_log_path)}_{'' if not convert_all else '_all'}.tif"


def build_parser():
    parser = argparse.ArgumentParser()
    add_parse_cmds_for_loaders(parser)
    add_parse_cmds_for_loggers(parser)
    add_parse_cmds_for_app(parser)
    return parser


def main(argv=None, backend=None, chunk=DEFAULT_CHUNK, generator=None):
    """generator: optional stand-in for the GeneratorChunks the CLI builds (tests)."""
    flags, _ = build_parser().parse_known_args(argv)
    mode, is_shadow, _ = parse_mode(flags.make_them_shadow)
    loader = get_loader_from_name(flags.loader_name, flags.path)
    data_set = loader.load_data(0, True)
    shadow_map, _ = loader.load_shadow_map(0, data_set)
    bands = data_set.get_casi_band_count()
    if bands < MIN_BANDS:
        raise ValueError(f"the shadow generator needs at least {MIN_BANDS} bands, the scene has {bands}")
    denorm_params(data_set)  # an unsupported dtype fails before the generator is built
    wrapper = get_infer_wrapper_dict()[flags.gan_type]
    if backend is None:
        from hypelcnn_amd.backend import HipBackend
        backend = HipBackend()
    if generator is None:
        generator = GeneratorChunks(wrapper, is_shadow, bands, backend)
        if mode != "none":  # reference :62-63: with `none` the freshly initialised generator runs
            variables = load_gan_variables(flags.base_log_path)
            generator.load({k: variables[k] for k in wrapper.create_generator_restorer()(list(variables))})
    start = time.time()
    image = convert_scene(data_set, shadow_map, mode, flags.convert_all, generator, backend, chunk=chunk,
                          rgb_band_measurements=loader.get_band_measurements() if flags.rgb else None)
    if flags.rgb:
        image, rgb = image
    os.makedirs(flags.output_path, exist_ok=True)
    path = os.path.join(flags.output_path, output_name(mode, flags.base_log_path, flags.convert_all))
    print(f"Saving output to {path}")
    imwrite(path, image)
    if flags.rgb:
        rgb_path = os.path.join(flags.output_path, rgb_output_name(mode, flags.base_log_path, flags.convert_all))
        print(f"Saving output RGB to {rgb_path}")
        imwrite(rgb_path, rgb)
    else:
        print("RGB rendering skipped: pass --rgb true for the sRGB rendering of the converted scene")
    print(f"Done conversion({time.time() - start:.3f} sec)")
    return image, path


if __name__ == "__main__":
    main()
