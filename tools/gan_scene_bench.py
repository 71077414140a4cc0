"""Whole-scene shadow conversion on the GRSS2013 geometry (349 x 1905 pixels, 144 bands): trains a CycleGAN for a few
steps, converts the scene in each mode and prints one JSON line with pixels/s and where the time goes (generator
chunks, de-normalise + scatter, host set-up and copy-back).  --rgb adds the sRGB rendering of the converted raster: the
hypel_hsi_to_srgb launch on the resident raster beside its byte floor (the span of bands it reads plus 3 bytes written
per pixel), and the float64 NumPy expression that launch replaces.

    python tools/gan_scene_bench.py [--steps 20] [--chunk 65536] [--dtype uint16] [--out DIR] [--rgb]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy  # noqa: E402
import torch  # noqa: E402

from hypelcnn_amd.backend import RGB_U8, HipBackend, Ref  # noqa: E402
from hypelcnn_amd.common import hsi_rgb_converter as HR  # noqa: E402
from hypelcnn_amd.gan import gan_infer_image_for_shadow as GI  # noqa: E402
from hypelcnn_amd.gan import gan_train_for_shadow as GT  # noqa: E402
from hypelcnn_amd.gan.gan_utilities import load_gan_variables  # noqa: E402
from hypelcnn_amd.gan.wrapper_registry import get_infer_wrapper_dict  # noqa: E402
from hypelcnn_amd.loader.SyntheticDataLoader import SyntheticDataLoader  # noqa: E402

SCENE = "grss2013:h=349:w=1905"  # the real GRSS2013 scene size: 664 845 pixels


HBM_BYTES_PER_S = 6.3e12  # what a float4 copy reaches on an MI355X


def numpy_render(band_measurements, image, casi_min, casi_max):
    """The reference's host expression on the package's table, float64: what the launch replaces."""
    r = (image.astype(float) - casi_min) / casi_max
    cmfs = HR.get_cmfs()
    xyz = (r[:, :, HR.select_visual_bands(band_measurements), None] * cmfs).sum(axis=2) / cmfs[:, 1].sum()
    m = numpy.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    lin = xyz @ numpy.linalg.inv(m).T
    with numpy.errstate(invalid="ignore"):
        rgb = numpy.where(lin > 0.0031308, 1.055 * numpy.power(lin, 1 / 2.4) - 0.055, 12.92 * lin)
    return (numpy.clip(rgb, 0, 1) * 255).astype(numpy.uint8)


def bench_rgb(backend, loader, ds, image, rounds=50):
    """Times `rounds` render launches between two device events, and the NumPy expression once.  The launches rotate
    over enough copies of the raster to exceed the 256 MiB Infinity Cache, so that each one reads from HBM."""
    h, w, bands = image.shape
    bm = loader.get_band_measurements()
    dtype, scale, offset = GI.denorm_params(ds)
    band0, span, table = HR.render_table(bm, bands, scale, offset)
    table_dev, levels, out = backend.upload(table), backend.upload(HR.srgb_levels()), backend.empty(h * w * 3, torch.uint8)
    copies = max(2, -(-(512 << 20) // image.nbytes))
    launches = [backend.bind("hsi_to_srgb", (Ref(backend.upload(image)), GI.OUT_DTYPES[dtype], bands, h * w, bands, band0,
                                             span, Ref(table_dev), Ref(levels), RGB_U8, Ref(out))) for _ in range(copies)]
    for launch in launches:
        launch()
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    for i in range(rounds):
        launches[i % copies]()
    end.record()
    torch.cuda.synchronize()
    launch_us = begin.elapsed_time(end) * 1e3 / rounds
    floor_bytes = h * w * (span * dtype.itemsize + 3)
    t0 = time.perf_counter()
    host = numpy_render(bm, image, ds.casi_min, ds.casi_max)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    got = out.cpu().numpy().reshape(h, w, 3)
    diff = numpy.abs(got.astype(numpy.int16) - host.astype(numpy.int16))
    return {"span_bands": span, "launch_us": round(launch_us, 2), "floor_bytes": floor_bytes,
            "floor_us": round(floor_bytes / HBM_BYTES_PER_S * 1e6, 2),
            "bytes_per_s": round(floor_bytes / (launch_us * 1e-6)), "numpy_float64_ms": round(numpy_ms, 1),
            "share_differing_from_numpy": float((diff != 0).mean()), "largest_difference": int(diff.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=GI.DEFAULT_CHUNK)
    ap.add_argument("--dtype", default="uint16")
    ap.add_argument("--out", default="/tmp/gan_scene_bench")
    ap.add_argument("--rgb", action="store_true", help="also time the sRGB rendering of the converted raster")
    args = ap.parse_args()
    scene = SCENE + ("" if args.dtype == "float32" else f":dtype={args.dtype}")
    backend = HipBackend()
    argv = ["--loader_name", "SyntheticDataLoader", "--path", scene, "--gan_type", "cycle_gan", "--batch_size", "1024",
            "--step", str(args.steps), "--base_log_path", os.path.join(args.out, "gan"), "--validation_steps", "1000000",
            "--validation_sample_count", "256"]
    params = dict(vars(GT.build_parser().parse_known_args(argv)[0]))
    GT.run_session(params, params["base_log_path"], backend=backend)
    log_dir = f"{params['base_log_path']}_{GT.get_log_suffix(type('F', (), params))}"
    ckpt = os.path.join(log_dir, f"model.ckpt-{args.steps}.npz")
    variables = load_gan_variables(ckpt)
    wrapper = get_infer_wrapper_dict()["cycle_gan"]
    loader = SyntheticDataLoader(scene)
    ds = loader.load_data(0, True)
    smap, _ = loader.load_shadow_map(0, ds)
    result = {"scene": scene, "pixels": int(smap.size), "bands": ds.get_casi_band_count(), "chunk": args.chunk,
              "modes": {}}
    for mode, convert_all in (("shadow", False), ("deshadow", False), ("shadow", True)):
        _, is_shadow, _ = GI.parse_mode(mode)
        gen = GI.GeneratorChunks(wrapper, is_shadow, ds.get_casi_band_count(), backend)
        gen.load({k: variables[k] for k in wrapper.create_generator_restorer()(list(variables))})
        GI.convert_scene(ds, smap, mode, convert_all, gen, backend, chunk=args.chunk)  # warm: phase compile, first use
        torch.cuda.synchronize()
        t = {}
        t0 = time.perf_counter()
        image = GI.convert_scene(ds, smap, mode, convert_all, gen, backend, chunk=args.chunk, timings=t,
                                 rgb_band_measurements=loader.get_band_measurements() if args.rgb else None)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if args.rgb:
            image = image[0]
        key = mode + ("_all" if convert_all else "")
        result["modes"][key] = {"converted": t["converted"], "wall_ms": round(wall * 1e3, 2),
                                "pixels_per_s": round(t["pixels"] / wall),
                                "converted_per_s": round(t["converted"] / max(t["generator_s"], 1e-9)),
                                "generator_ms": round(t["generator_s"] * 1e3, 2),
                                "denorm_ms": round(t["denorm_s"] * 1e3, 2),
                                "passthrough_denorm_ms": round(t["passthrough_s"] * 1e3, 3),
                                "host_setup_ms": round(t["setup_s"] * 1e3, 2),
                                "copy_back_ms": round(t["copy_back_s"] * 1e3, 2)}
        if args.rgb:  # launch, host synchronisation and the copy of the 3-byte pixels
            result["modes"][key]["rgb_ms"] = round(t["rgb_s"] * 1e3, 3)
    if args.rgb:
        result["rgb"] = bench_rgb(backend, loader, ds, image)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
