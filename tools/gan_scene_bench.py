"""Whole-scene shadow conversion on the GRSS2013 geometry (349 x 1905 pixels, 144 bands): trains a CycleGAN for a few
steps, converts the scene in each mode and prints one JSON line with pixels/s and where the time goes (generator
chunks, de-normalise + scatter, host set-up and copy-back).

    python tools/gan_scene_bench.py [--steps 20] [--chunk 65536] [--dtype uint16] [--out DIR]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from hypelcnn_amd.backend import HipBackend  # noqa: E402
from hypelcnn_amd.gan import gan_infer_image_for_shadow as GI  # noqa: E402
from hypelcnn_amd.gan import gan_train_for_shadow as GT  # noqa: E402
from hypelcnn_amd.gan.gan_utilities import load_gan_variables  # noqa: E402
from hypelcnn_amd.gan.wrapper_registry import get_infer_wrapper_dict  # noqa: E402
from hypelcnn_amd.loader.SyntheticDataLoader import SyntheticDataLoader  # noqa: E402

SCENE = "grss2013:h=349:w=1905"  # the real GRSS2013 scene size: 664 845 pixels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=GI.DEFAULT_CHUNK)
    ap.add_argument("--dtype", default="uint16")
    ap.add_argument("--out", default="/tmp/gan_scene_bench")
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
        GI.convert_scene(ds, smap, mode, convert_all, gen, backend, chunk=args.chunk, timings=t)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        key = mode + ("_all" if convert_all else "")
        result["modes"][key] = {"converted": t["converted"], "wall_ms": round(wall * 1e3, 2),
                                "pixels_per_s": round(t["pixels"] / wall),
                                "converted_per_s": round(t["converted"] / max(t["generator_s"], 1e-9)),
                                "generator_ms": round(t["generator_s"] * 1e3, 2),
                                "denorm_ms": round(t["denorm_s"] * 1e3, 2),
                                "passthrough_denorm_ms": round(t["passthrough_s"] * 1e3, 3),
                                "host_setup_ms": round(t["setup_s"] * 1e3, 2),
                                "copy_back_ms": round(t["copy_back_s"] * 1e3, 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
