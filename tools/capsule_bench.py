"""CAPModel training step at the shipped configuration (GRSS2013 7x7x145, 15 classes, tests/golden/alg_param_capn.json):
one JSON line with the captured step time at batch 16 and 256 and, per capsule launch, its time (eager, event-timed,
median) next to its byte-count floor -- the launch's bytes / 6.2 TB/s, the streaming rate DESIGN.md uses for the
element-wise passes.

    python tools/capsule_bench.py [--steps 50] [--warmup 10] [--batches 16,256]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hypelcnn_amd.backend import HipBackend  # noqa: E402
from hypelcnn_amd.common import common_nn_ops as cno  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_BYTES_PER_S = 6.2e12


def build(backend, alg, nb):
    model = cno.get_model_from_name("CAPModel")
    template = cno.Template("nn_core", model.create_tensor_graph, class_count=15)
    ctx = cno.GraphContext(template, backend)
    images, labels = cno.Placeholder("x", (7, 7), 145), cno.Placeholder("labels", None, 15)
    _, _, lr, train_step = cno.optimize_nn(template, images, labels, "/gpu:0", "training", alg, model.get_loss_func, ctx=ctx)
    ct = train_step.compiled(nb)
    rng = np.random.default_rng(0)
    ct.set_input("x", torch.from_numpy(rng.random((nb, 7, 7, 145)).astype(np.float32)).to(backend.device))
    ct.set_input("labels", torch.from_numpy(np.eye(15, dtype=np.float32)[rng.integers(0, 15, nb)]).to(backend.device))
    return ctx.session(), ct, lr


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream())
        fn()
        b.record(torch.cuda.current_stream())
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", default="16,256")
    args = ap.parse_args()
    alg = json.load(open(os.path.join(ROOT, "tests", "golden", "alg_param_capn.json")))
    backend = HipBackend()
    result = {"tool": "capsule_bench", "config": "grss2013 7x7x145, 15 classes, alg_param_capn.json", "batches": {}}
    for nb in [int(v) for v in args.batches.split(",")]:
        sess, ct, lr = build(backend, alg, nb)

        def step():
            ct.forward_backward()
            sess.adam_step(lr.eval(0))
        entry = {"step_us": round(timed(step, args.steps, args.warmup), 1), "launches": []}
        for launch, call in ct.serial_launches():
            if not launch.name.startswith("caps_"):
                continue
            us = timed(call, max(10, args.steps // 2), 3)
            floor = launch.bytes / STREAM_BYTES_PER_S * 1e6
            entry["launches"].append({"name": launch.name, "tag": launch.tag, "us": round(us, 1),
                                      "floor_us": round(floor, 2), "x_floor": round(us / floor, 1) if floor else None})
        result["batches"][str(nb)] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
