#!/usr/bin/env python3
"""Headline benchmark: HSI+LiDAR patches/sec, forward+backward+optimiser, GRSS2013 HYPELCNN
(7x7x(144+1), 15 classes, alg_param_hypelcnn.json), batch 1024 per GPU, fp32 -- BASELINE.json configs[1].

  python bench.py --gpus N --steps K --warmup W        (N>1: launched by torch.distributed.run, one rank per GPU)
  python bench.py ... --dump-outputs DIR              (also write what the last timed step computed to DIR/*.npy)
  python bench.py ... --full                          (also every secondary figure and check, see below)

A "step" = next resident batch -> nhwc->pixel-major -> forward -> loss -> backward -> (RCCL all-reduce)
-> TF1-Adam.  Inputs are synthetic (U[0,1) patches, uniform labels) and already resident in HBM.
Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times the K steps,
dumps (if asked) and prints the line; `roofline` and `cpu_baseline` are null in it.  --full adds, after the timed
steps: `roofline` for the dominant kernel (hypel_seg_gemm_f32: HIP events over an eager replay, clock / power over an
untimed replay), `with_input_pipeline` (hypelcnn), the data-parallel weight check, and `cpu_baseline` (oracle
restatement timed on the host cores).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
# fp32-equivalent peak of the split-operand kernels: six v_mfma_f32_32x32x16_bf16 per fp32 multiply-add step against the
# dense bf16 peak of the same guide (~2.5 PFLOP/s; AMD's 5 PF headline includes 2:1 sparsity and is never used here)
PEAK_SPLIT6_TFLOPS = 2500.0 / 6
MAC_FWD_PER_PATCH = 78579058  # SURVEY.md Appendix B.1 (exact taps, training graph)


CLASSIFIER_WORKLOADS = {
    # name: (model, alg json, patch, channels, classes, default batch/GPU, exact fwd MAC per patch)
    "hypelcnn": ("HYPELCNNModel", "alg_param_hypelcnn.json", 7, 145, 15, 1024, 78579058),
    "dualcnn": ("DUALCNNModel", "alg_param_dualcnn.json", 11, 49, 20, 512, None),
}

# --dump-outputs: the pre-warm is this fixed number of steps instead of one derived from a timing, so that the state the
# timed steps start from (weights, optimiser moments, step count, dropout draws) depends on the arguments only.  Each covers
# the 50 ms of work the shader clock needs to ramp at the workload's default batch (step times of DESIGN.md 5).
DUMP_PREWARM_STEPS = {"hypelcnn": 12, "dualcnn": 2, "cyclegan": 250, "cut": 45}
DUMP_MAX_ELEMENTS = 4 << 20  # per array (16 MB of float32): larger outputs are written as a fixed, seeded sample


def dump_outputs(directory, arrays):
    """Write {name: array} as DIR/<name>.npy (float32, or float64 for the float64 scalars): arrays above DUMP_MAX_ELEMENTS
    are flattened and sampled at positions drawn by a fixed seed from their size alone, the same in every run and build.
    Returns {name: [shape written, shape computed]}."""
    os.makedirs(directory, exist_ok=True)
    written = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
        shape = list(a.shape)
        if a.size > DUMP_MAX_ELEMENTS:
            idx = np.sort(np.random.default_rng(0).choice(a.size, DUMP_MAX_ELEMENTS, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(directory, name + ".npy"), a)
        written[name] = [list(a.shape), shape]
    return written


def build_model(batch, backend, workload="hypelcnn"):
    from hypelcnn_amd.common import common_nn_ops as cno
    name, cfg, patch, chans, classes, _, _ = CLASSIFIER_WORKLOADS[workload]
    alg = json.load(open(os.path.join(ROOT, "hypelcnn_amd", "nnmodel", "modelconfigs", cfg)))
    alg["batch_size"] = batch
    model = cno.get_model_from_name(name)
    template = cno.Template("nn_core", model.create_tensor_graph, class_count=classes)
    ctx = cno.GraphContext(template, backend)
    images = cno.Placeholder("x", (patch, patch), chans)
    labels = cno.Placeholder("labels", None, classes)
    _, cross_entropy, lr, train_step = cno.optimize_nn(template, images, labels, "/gpu:0", "training", alg,
                                                       model.get_loss_func, ctx=ctx)
    return ctx, train_step, lr, alg


def is_split6(l):
    """A seg_gemm launch on the split-operand kernels (include/hypel.h: HYPEL_GEMM_SPLIT6 in `accumulate` /
    HYPEL_GEMM_MULTI_SPLIT6 in tile_width)."""
    return bool(l.args[3] & 0x100) if l.name == "seg_gemm_multi_f32" else bool(l.args[14] & 0x8000)


def split6_flop_share(ct):
    """(share of the step's seg_gemm FLOP on the split-operand kernels, number of such launches) from the plan alone:
    no launch runs."""
    gl = [l for l in ct.plan.fwd + ct.plan.bwd if l.name.startswith("seg_gemm")]
    return sum(l.flops for l in gl if is_split6(l)) / max(1, sum(l.flops for l in gl)), sum(1 for l in gl if is_split6(l))


def measure_gemm_events(ct, sess, lr, steps):
    """Serial replay of the same step (every launch on the main stream, no graph) with a HIP event pair around
    every hypel_seg_gemm_f32 launch, recorded on the stream the kernels are launched on."""
    launches = ct.serial_launches()
    total_ms, total_flops, n_launch = 0.0, 0, 0
    measure_gemm_events.bytes_per_launch = (sum(l.bytes for l, _ in launches if l.name.startswith("seg_gemm")) /
                                            max(1, sum(1 for l, _ in launches if l.name.startswith("seg_gemm"))))
    for _ in range(steps):
        evs = []
        for l, f in launches:
            if l.name.startswith("seg_gemm"):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                evs.append((a, b, l.flops))
            else:
                f()
        sess.adam_step(lr.eval(sess.global_step))
        torch.cuda.synchronize()
        total_ms += sum(a.elapsed_time(b) for a, b, _ in evs)
        n_launch += len(evs)
        total_flops += sum(fl for _, _, fl in evs)
    measure_gemm_events.split_flop_share, measure_gemm_events.split_launches = split6_flop_share(ct)
    return total_ms, total_flops, n_launch


def _cpu_numpy_oracle(alg, nb, seconds_budget):
    from oracle import models as OM, train as OT
    rng = np.random.default_rng(1234)
    params = OM.hypelcnn_init_params(7, 145, 15, alg, rng, np.float32)
    tr = OT.ClassifierTrainer("HYPELCNNModel", params, 15, alg)
    x = rng.random((nb, 7, 7, 145), dtype=np.float32)
    onehot = np.eye(15, dtype=np.float32)[rng.integers(0, 15, nb)]
    tr.train_step(x, onehot)  # warm-up
    t0 = time.perf_counter()
    n = 0
    while True:
        tr.train_step(x, onehot)
        n += 1
        if time.perf_counter() - t0 > seconds_budget or n >= 50:
            break
    return nb * n / (time.perf_counter() - t0), n


def _cpu_torch_oracle(alg, nb, seconds_budget, workload="hypelcnn", max_steps=200):
    """oracle/torch_ref.py: the same graph as a torch-CPU (oneDNN/MKL) autograd composition + torch Adam with the
    TF1 epsilon placement folded into lr_t -- the closest stand-in for the reference's TF-CPU path."""
    from oracle import models as OM, torch_ref as TR
    _, _, patch, chans, classes, _, _ = CLASSIFIER_WORKLOADS[workload]
    rng = np.random.default_rng(1234)
    if workload == "hypelcnn":
        params = OM.hypelcnn_init_params(patch, chans, classes, alg, rng, np.float32)
    else:
        params = OM.xavier_init_params(OM.dualcnn_layer_table(patch, chans, classes, alg), rng, np.float32)
    P = {k: torch.tensor(v, requires_grad=not k.endswith(("moving_mean", "moving_variance")))
         for k, v in params.items()}
    train = [v for v in P.values() if v.requires_grad]
    m = [torch.zeros_like(v) for v in train]
    vv = [torch.zeros_like(v) for v in train]
    x = torch.tensor(rng.random((nb, patch, patch, chans), dtype=np.float32))
    onehot = torch.tensor(np.eye(classes, dtype=np.float32)[rng.integers(0, classes, nb)])
    step = [0]

    def one():
        if workload == "hypelcnn":
            out = TR.hypelcnn(P, x, classes, alg, True, masks=None)
            loss = TR.hypelcnn_loss(out[0], out[1], x, onehot).mean()
        else:
            logits = TR.dualcnn(P, x, classes, alg, True, masks=None)
            logits = logits[0] if isinstance(logits, tuple) else logits
            loss = -(onehot * torch.log_softmax(logits, 1)).sum(1).mean()
        grads = torch.autograd.grad(loss, train)
        step[0] += 1
        t = step[0]
        lr_t = alg["learning_rate"] * (1 - 0.999 ** t) ** 0.5 / (1 - 0.9 ** t)
        with torch.no_grad():
            torch._foreach_mul_(m, 0.9)
            torch._foreach_add_(m, grads, alpha=0.1)
            torch._foreach_mul_(vv, 0.999)
            torch._foreach_addcmul_(vv, grads, grads, value=0.001)
            den = torch._foreach_sqrt(vv)
            torch._foreach_add_(den, 1e-8)
            torch._foreach_addcdiv_(train, m, den, value=-lr_t)
    one()
    t0 = time.perf_counter()
    n = 0
    while True:
        one()
        n += 1
        if time.perf_counter() - t0 > seconds_budget or n >= max_steps:
            break
    return nb * n / (time.perf_counter() - t0), n


def _thread_sweep(fn, counts):
    """fn() under each torch thread count: (best result, its thread count, {threads: value})."""
    default_threads = torch.get_num_threads()
    best, best_nt, table = (0.0, 0), None, {}
    for nt in counts:
        torch.set_num_threads(nt)
        r = fn()
        table[nt] = round(r[0], 1)
        if r[0] > best[0]:
            best, best_nt = r, nt
    torch.set_num_threads(default_threads)
    return best, best_nt, table


def cpu_baseline(seconds_budget=12.0, workload="hypelcnn"):
    """The identical train step restated on the host cores, on bounded samples (SURVEY 8d asks for both shapes):
    batch 64 (BASELINE configs[0], the reference's own CPU-runnable case) and the benchmark's batch (configs[1]: 1024).
    Restatements: the numpy oracle (oracle/train.py, batch 64 only) and the torch-CPU composition (oracle/torch_ref.py)
    under a sweep of thread counts up to the host's logical cores; the FASTEST figure is `value`, `cores` the threads
    that produced it.  DUALCNN: the torch-CPU composition at batch 16."""
    cfg = CLASSIFIER_WORKLOADS[workload][1]
    alg = json.load(open(os.path.join(ROOT, "hypelcnn_amd", "nnmodel", "modelconfigs", cfg)))
    cores = os.cpu_count() or 8
    # thread sweep: oversubscribed pools collapse on these small convolutions (MI355X host, 256 logical cores, round-5
    # profile run: 834 / 184 / 0.5 patches/s at 16 / 64 / 256 threads, batch 64 -- a single 256-thread step took minutes),
    # so the sweep stops at 64 threads and the default bench run stays within its few minutes
    counts = sorted({min(16, cores), min(32, cores), min(64, cores)})
    if workload == "dualcnn":
        try:
            best, nt, table = _thread_sweep(lambda: _cpu_torch_oracle(alg, 16, seconds_budget / len(counts), "dualcnn", 50), counts)
        except Exception as e:
            print(f"bench.py: torch-CPU baseline failed: {e!r}", file=sys.stderr)
            return None
        return {"value": best[0], "unit": "patches/s", "cores": nt, "kind": "port",
                "sample": f"{best[1]} train steps of batch 16 (11x11x49, fp32) with the torch-CPU (oneDNN) composition of the "
                          f"reference graph (oracle/torch_ref.py); thread sweep {table} patches/s; host has {cores} logical "
                          f"cores; not a TensorFlow number"}
    res = {"numpy": _cpu_numpy_oracle(alg, 64, seconds_budget / 2)}
    torch_threads, t64, t1024, nt1024 = None, {}, {}, None
    b1024 = (0.0, 0)
    try:
        res["torch_cpu"], torch_threads, t64 = _thread_sweep(
            lambda: _cpu_torch_oracle(alg, 64, seconds_budget / (2 * len(counts))), counts)
        b1024, nt1024, t1024 = _thread_sweep(lambda: _cpu_torch_oracle(alg, 1024, seconds_budget / len(counts), max_steps=8), counts)
    except Exception as e:  # the torch leg is optional evidence; never fail the bench line on it
        print(f"bench.py: torch-CPU baseline failed: {e!r}", file=sys.stderr)
        res.setdefault("torch_cpu", (0.0, 0))
    best = max(res, key=lambda k: res[k][0])
    value, used = res[best][0], (torch_threads if best == "torch_cpu" else cores)
    shape = "batch 64"
    if b1024[0] > value:
        value, used, shape, best = b1024[0], nt1024, "batch 1024", "torch_cpu"
    return {"value": value, "unit": "patches/s", "cores": used, "kind": "port",
            "batch_64": {"numpy_oracle": round(res["numpy"][0], 1), "torch_cpu_by_threads": t64},
            "batch_1024": {"torch_cpu_by_threads": t1024},
            "sample": f"fastest of: {res['numpy'][1]} train steps of batch 64 (7x7x145, fp32) with the numpy/OpenBLAS oracle; "
                      f"the torch-CPU (oneDNN) composition at batch 64 and at batch 1024 (<= 8 steps) under "
                      f"{counts} threads -- reported: {best} at {shape} with {used} threads; host has {cores} logical "
                      f"cores; not a TensorFlow number"}


def baseline_metric():
    """The metric name exactly as BASELINE.json spells it (the driver matches the bench line against it)."""
    try:
        return json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    except (OSError, KeyError, ValueError):
        return "HSI+LiDAR patches/sec fwd+bwd (GRSS2013 7\u00d77\u00d7145) at 1/2/4/8 GPU"


def source_fingerprint():
    """sha256 over the tracked source files of the product path (relative path + content).  tools/gpu.sh stores it next
    to the commit hash in .head_commit (the GPU snapshot has no .git); a .head_commit whose fingerprint does not match
    the files this process runs from is stale and is NOT printed."""
    import hashlib
    h = hashlib.sha256()
    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "include", "hypel.h")]
    for base, _, names in os.walk(os.path.join(ROOT, "hypelcnn_amd")):
        if "build" in base.split(os.sep) or "alt" in base.split(os.sep) or "__pycache__" in base:
            continue
        files += [os.path.join(base, n) for n in names if n.endswith((".py", ".hip", ".h", ".cpp", ".json")) or n == "Makefile"]
    for f in sorted(files):
        h.update(os.path.relpath(f, ROOT).encode())
        with open(f, "rb") as fh:
            h.update(hashlib.sha256(fh.read()).digest())
    return h.hexdigest()[:16]


PRODUCT_PATHS = "hypelcnn_amd include bench.py"  # what source_fingerprint() covers


def commit_label():
    """Short hash of the code this process runs: from git when the tree has a .git (suffix +dirty when tracked files
    differ), else from .head_commit -- only when its fingerprint matches the files on disk."""
    # the last commit that touches the product path (later documentation / profile commits do not change what runs)
    commit = os.popen(f"git -C {ROOT} log -1 --format=%h -- {PRODUCT_PATHS} 2>/dev/null").read().strip()
    if commit:
        dirty = os.popen(f"git -C {ROOT} status --porcelain --untracked-files=no -- {PRODUCT_PATHS} 2>/dev/null").read().strip()
        return commit + ("+dirty" if dirty else ""), None
    try:
        parts = open(os.path.join(ROOT, ".head_commit")).read().split()
    except OSError:
        return None, "no .git and no .head_commit"
    if len(parts) >= 2 and parts[1] == source_fingerprint():
        return parts[0], None
    return None, "stale .head_commit (source fingerprint differs): not printed"


def generator_exact_macs(bands, only_encoder):
    """Exact-tap multiply-adds of one generator application per sample (384 244 at B = 360)."""
    tot = 0
    for sh in (0, 1, 2, 3, 2, 1, 0)[: 4 if only_encoder else 7]:
        k = bands >> sh
        p = (k - 1) // 2
        tot += sum(min(bands - 1, j + k - 1 - p) - max(0, j - p) + 1 for j in range(bands))
    return tot


def measure_gan_events(ops, nb, bands, steps):
    """Eager replay of every phase of the GAN step with a HIP event pair around each generator launch (forward:
    2 * MAC FLOP per sample; backward = data gradient + filter gradient: 4 * MAC -- the backward pass starts from the
    activations its forward pass kept, and a recompute would not be algorithmic work anyway).  Also counts the
    launches of a step (kernel boundaries are what bounds the B = 64 stacks)."""
    sess = ops.ctx.session()
    towers = list(sess._compiled.values())
    lists = [ct.serial_launches() for ct in towers]
    n_launch = sum(len(l) for l in lists) + sum(len(sess._merged_ranges(ph.train_groups)) for ph in ops.loss.phases)
    ms, flops, n_gen = 0.0, 0.0, 0
    for _ in range(steps):
        evs = []
        for launches in lists:
            for l, f in launches:
                if l.name.startswith("gan_generator"):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    f()
                    b.record()
                    bwd = "_bwd" in l.name  # gan_generator_bwd / _bwd_kept / _bwd_tap / _bwd_apps
                    if l.name.endswith("_tap"):
                        # the full generator whose n_4 doubles as the encoder-only application on the same input: its
                        # algorithmic work is the full generator's (the shared encoder layers are computed once)
                        enc, rows = False, int(l.args[6] if bwd else l.args[2])
                    elif l.name.endswith("_apps"):
                        # several same-shaped generators, each on `n` rows of the launch (hypel.h: *_apps)
                        enc = bool(l.args[13] if bwd else l.args[9])
                        rows = int(l.args[4] if bwd else l.args[2]) * int(l.args[5] if bwd else l.args[3])
                    else:
                        enc = bool(l.args[8] if bwd else l.args[6])
                        rows = int(l.args[4] if bwd else l.args[2])  # k * nb when k same-weight applications run as one
                    evs.append((a, b, (4 if bwd else 2) * generator_exact_macs(bands, enc) * rows))
                else:
                    f()
        torch.cuda.synchronize()
        ms += sum(a.elapsed_time(b) for a, b, _ in evs)
        flops += sum(fl for _, _, fl in evs)
        n_gen += len(evs)
    return ms / steps, flops / steps, n_gen // steps, n_launch


def gan_cpu_baseline(kind, bands, seconds_budget=12.0):
    """oracle/gan.py::GanTrainer (numpy restatement of the wrapper's sequential train ops + TF1 Adam) on a bounded
    sample: as many steps of a small batch as fit the budget."""
    from oracle import gan as OG
    rng = np.random.default_rng(1234)
    nb = 256 if bands <= 64 else 32
    cfg = OG.GanConfig(kind, bands)
    params = OG.init_gan_params(kind, bands, rng)
    tr = OG.GanTrainer(cfg, params)
    x = rng.random((nb, 1, 1, bands), dtype=np.float32)
    y = (x / (1.0 + rng.random((1, 1, 1, bands), dtype=np.float32))).astype(np.float32)
    tr.step(x, y)
    t0 = time.perf_counter()
    n = 0
    while True:
        tr.step(x, y)
        n += 1
        if time.perf_counter() - t0 > seconds_budget or n >= 200:
            break
    dt = time.perf_counter() - t0
    return {"value": nb * n / dt, "unit": "pairs/s", "cores": os.cpu_count(), "kind": "port",
            "sample": f"{n} full {kind} steps (all sequential train ops + TF1 Adam) of {nb} pairs x {bands} bands with the "
                      f"numpy restatement oracle/gan.py::GanTrainer (numpy/OpenBLAS threads: host has {os.cpu_count()} "
                      f"logical cores); not a TensorFlow number"}


class ClockSampler:
    """Shader clock (and socket power) of this rank's GPU while the workload's steps run (an untimed replay), read from sysfs every few milliseconds by
    a host thread (amdgpu: pp_dpm_sclk marks the current level with '*', hwmon power1_average is in microwatts) -- the
    driver-visible record behind `roofline.peak_note`: the split kernels run against the power cap, i.e. below the 2.4 GHz
    the peak assumes.  Values are None where the files do not exist."""

    @staticmethod
    def _pci_address(index):
        """PCI address ("0000:75:00.0") of HIP device `index` of this process -- the node's OTHER GPUs (other tenants' work) are
        visible in sysfs too, and card numbers do not follow HIP's device order.  From torch's device properties: no second
        handle on the HIP runtime, no failed query that stays behind as its sticky error."""
        try:
            import torch
            p = torch.cuda.get_device_properties(int(index))
            return f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
        except Exception:  # noqa: BLE001 -- a diagnostic field, never a reason to fail the bench
            return None

    def __init__(self, index=0, period=0.004):
        import glob
        devs = sorted(glob.glob("/sys/class/drm/card[0-9]*/device"))
        addr = self._pci_address(index)
        mine = [d for d in devs if addr and os.path.basename(os.path.realpath(d)).lower() == addr]
        self.matched_by = "pci address" if mine else ("only card" if len(devs) == 1 else "not identified")
        dev = mine[0] if mine else (devs[0] if len(devs) == 1 else None)  # never guess among several GPUs
        self.sclk = os.path.join(dev, "pp_dpm_sclk") if dev and os.path.exists(os.path.join(dev, "pp_dpm_sclk")) else None
        pw = (sorted(glob.glob(os.path.join(dev, "hwmon/hwmon*/power1_average"))) or
              sorted(glob.glob(os.path.join(dev, "hwmon/hwmon*/power1_input")))) if dev else []
        self.power = pw[0] if pw else None
        # hwmon freq1_input = the current shader clock in Hz; boxes of this pool whose level table is pinned at its top entry
        # (a constant 2 400 MHz from pp_dpm_sclk whatever runs) still move here
        fq = sorted(glob.glob(os.path.join(dev, "hwmon/hwmon*/freq1_input"))) if dev else []
        self.freq = fq[0] if fq else None
        self.period, self.mhz, self.watts, self.hz, self._stop, self._t = period, [], [], [], False, None

    def _run(self):
        import re
        while not self._stop:
            try:
                m = re.search(r"(\d+)\s*[Mm][Hh]z\s*\*", open(self.sclk).read())
                if m:
                    self.mhz.append(int(m.group(1)))
                if self.power:
                    self.watts.append(int(open(self.power).read()) / 1e6)
                if self.freq:
                    self.hz.append(int(open(self.freq).read()))
            except (OSError, ValueError):
                pass
            time.sleep(self.period)

    def __enter__(self):
        if self.sclk and os.environ.get("HYPEL_BENCH_CLOCK", "1") != "0":
            import threading
            self._t = threading.Thread(target=self._run, daemon=True)
            self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        if self._t:
            self._t.join(timeout=1.0)
        return False

    def summary(self):
        mean = lambda v: (sum(v) / len(v)) if v else None  # noqa: E731
        ghz = mean(self.mhz)
        hw = mean(self.hz)
        return {"sustained_clock_ghz": None if ghz is None else ghz / 1e3,
                "sustained_clock_hwmon_ghz": None if hw is None else hw / 1e9,
                "sustained_clock_min_max_ghz": [min(self.mhz) / 1e3, max(self.mhz) / 1e3] if self.mhz else None,
                "sustained_power_w": mean(self.watts), "clock_samples": len(self.mhz),
                "clock_source": "sysfs pp_dpm_sclk (current level) / hwmon freq1_input / hwmon power1_average|input of this rank's GPU "
                                f"({self.matched_by}), sampled every 4 ms over an untimed replay of the timed steps"}


TRAFFIC_SUMMARIES = ("r6_hbm_traffic.json", "r6_hbm_traffic_dualcnn.json", "r5_hbm_traffic.json", "r5_hbm_traffic_dualcnn.json", "r4_hbm_traffic.json", "r4_hbm_traffic_dualcnn.json", "r3_hbm_traffic.json", "r3_hbm_traffic_dualcnn.json", "r2_hbm_traffic.json", "r1_hbm_traffic.json")


def pmc_traffic(workload, nb, launches_per_step):
    """HBM bytes per seg_gemm launch from the PMC passes of this same command (FETCH_SIZE and WRITE_SIZE need
    separate rocprofv3 passes, so they cannot be collected inside the bench run): read from the newest committed
    summary under profiles/ (tools/pmc_traffic.py; corrections per MI355X_MICROARCH.md) that describes this
    workload, batch and launch structure.  Returns (bytes per launch or None, source label)."""
    for name in TRAFFIC_SUMMARIES:
        path = os.path.join(ROOT, "profiles", name)
        try:
            d = json.load(open(path))
        except (OSError, ValueError):
            continue
        if d.get("workload") != workload or d.get("batch") != nb:
            continue
        if "seg_gemm_bytes_per_step" in d:  # launch structure changed since the PMC pass: re-express per launch
            return d["seg_gemm_bytes_per_step"] / max(1, launches_per_step), f"profiles/{name} (committed PMC passes)"
        if d.get("seg_gemm_launches_per_step", launches_per_step) == launches_per_step:
            return d["seg_gemm_bytes_per_launch"], f"profiles/{name} (committed PMC passes)"
    return None, None


def pmc_mfma_busy(workload):
    """Matrix-pipe busy share of the seg_gemm launches from the committed SQ-counter pass of this same command
    (tools/pmc_sq_per_launch.py: SQ_VALU_MFMA_BUSY_CYCLES against GRBM_GUI_ACTIVE; its own rocprofv3 run).  Returns
    ({"busy": ..., "useful": ...} or None, source label)."""
    import re
    last = None
    for tag in ("r6", "r5"):
        name = f"{tag}_mfma_busy_per_launch_{workload}.txt"
        try:
            last = open(os.path.join(ROOT, "profiles", name)).read().strip().splitlines()[-1]
            break
        except OSError:
            continue
    if last is None:
        return None, None
    m = re.search(r"mfma busy ([0-9.]+) % .* useful ([0-9.]+) %", last)
    if not m:
        return None, None
    return {"busy": float(m.group(1)) / 100, "useful": float(m.group(2)) / 100}, f"profiles/{name} (committed PMC pass)"


def input_pipeline_iterator(be, nb, patch, chans, classes, rank, pool=8192):
    """The reference's tf.data stage (common/common_nn_ops.py:188-201,376-440) for the timed loop: a resident pool
    of `pool` synthetic patches, per-epoch permutation, per-sample rot90 / flips / spectral shift drawn on the device
    and applied by ONE hypel_augment_patches_f32 launch that also gathers the batch."""
    from hypelcnn_amd.common import common_nn_ops as cno
    gen = torch.Generator(device="cpu")
    gen.manual_seed(4321 + rank)
    data = torch.rand((pool, patch, patch, chans), generator=gen).numpy()
    labels = torch.randint(0, classes, (pool,), generator=gen).numpy()
    info = cno.AugmentationInfo(None, False, True, 0.05, True, 0.5)
    it = cno.BatchIterator((patch, patch, chans), classes, nb, True, None, info)
    it.initializer(data, labels, be)
    return it


def run_gan_workload(args, be, world, rank):
    """cfg4 (CycleGAN, [N,1,1,64] pairs) / GAN half of cfg5 (CUT, [N,1,1,360]): one step = every sequential train
    op of the wrapper (generator phase, discriminator phase, (feature-discriminator phase)) incl. Adam.  These
    stacks are launch-latency / HBM bound: the line reports pairs/s and the algorithmic GB/s."""
    from types import SimpleNamespace
    from hypelcnn_amd.gan.wrapper_registry import get_wrapper_dict
    from hypelcnn_amd.gan.wrappers import gan_common as C
    kind, bands = ("cycle_gan", 64) if args.workload == "cyclegan" else ("cut_x2y", 360)
    nb = args.batch or (2048 if kind == "cycle_gan" else 4096)
    flags = SimpleNamespace(discriminator_reg_scale=1e-5, gen_disc_reg_scale=1e-4, embedded_feat_size=2, patches=6,
                            cycle_consistency_loss_weight=10.0, identity_loss_weight=0.5, use_identity_loss=True,
                            nce_loss_weight=10.0, tau=0.07, batch_size=nb)
    wrapper = get_wrapper_dict(flags)[kind]
    wrapper.backend = be
    tower, xs, ys = C.new_gan_tower(bands)
    model = wrapper.define_model(xs, ys)
    loss = wrapper.define_loss(model)
    ops = wrapper.define_train_ops(model, loss, max_number_of_steps=100000, generator_lr=2e-4,
                                   discriminator_lr=1e-4, gen_discriminator_lr=1e-4)
    ops.capture_graphs = not args.no_graph
    sess = ops.ctx.session()
    # the reference zero-initialises the generator (shadow_data_models.py:62-86), which makes every step trivial
    # numerically but not computationally; keep it
    gen = torch.Generator(device="cpu")
    gen.manual_seed(1234 + rank)
    x = torch.rand((nb, bands), generator=gen).cuda()
    y = (x / (1.0 + torch.rand((1, bands), generator=gen).cuda())).contiguous()
    return nb, bands, kind, (lambda: ops.run_step(x, y)), (lambda: float(sum(ops.losses().values()))), ops


def prewarm_by_time(one_step, use_dist, note_collective):
    """Run at least 50 ms of steps; returns how many ran.  Every rank must run the SAME number of steps -- a step ends in
    collectives -- so the count is derived from three timed steps and, under data parallelism, agreed on by a MAX
    all-reduce."""
    import torch.distributed as dist
    tw = time.perf_counter()
    for _ in range(3):
        one_step()
    torch.cuda.synchronize()
    est = (time.perf_counter() - tw) / 3
    n_prewarm = max(2, min(500, int(0.05 / max(est, 1e-6)) + 1))
    if use_dist:
        t = torch.tensor([n_prewarm], device="cuda", dtype=torch.int32)
        note_collective()  # a later HIP-graph capture must wait this collective out (backend.settle_before_capture)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        n_prewarm = int(t[0])
    for _ in range(n_prewarm):
        one_step()
    return n_prewarm + 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=0, help="samples per GPU per step (0 = the workload's default)")
    ap.add_argument("--workload", default="hypelcnn", choices=["hypelcnn", "dualcnn", "cyclegan", "cut"],
                    help="hypelcnn = BASELINE.json headline (configs[1]); the others are extra evidence lines")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything the headline does not need: roofline "
                         "(HIP-event replay, clock / power), input-pipeline step, data-parallel weight check, CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of HIP-graph replay")
    ap.add_argument("--sync-bn", action="store_true",
                    help="N > 1: batch-norm statistics over the global batch (one small RCCL collective per BN layer and "
                         "direction; default: per-rank statistics)")
    ap.add_argument("--no-input-pipeline", action="store_true",
                    help="--full without the second measurement (step fed by the device BatchIterator + augmentation kernel)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (loss, logits / per-phase losses, "
                         "updated weights, gradients) to DIR/<name>.npy; the pre-warm becomes a fixed step count so "
                         "that runs with the same arguments compute the same outputs")
    args = ap.parse_args()
    if args.sync_bn:
        os.environ["HYPEL_SYNC_BN"] = "1"  # read by Session.init_data_parallel

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # bare `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU, rendezvous on 127.0.0.1) by
        # re-executing this command under torch.distributed.run; rank 0 of that job prints the one JSON line
        import socket
        import subprocess
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL / cross-process tensors on this driver)
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd, env=env))
    if args.gpus > 1 and world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    # HYPEL_DIST_BACKEND=gloo: rehearse the N > 1 flow on a box with fewer GPUs than ranks (ranks share devices;
    # RCCL refuses that).  The driver's runs use nccl (= RCCL), one rank per GPU.
    backend_name = os.environ.get("HYPEL_DIST_BACKEND", "nccl")
    if backend_name != "nccl":
        local_rank %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    import torch.distributed as dist
    # HYPEL_DP_SELFTEST=1 under `torch.distributed.run --nproc-per-node 1`: drive the whole RCCL path on a 1-rank
    # communicator (the only multi-process GPU check a 1-GPU box allows)
    use_dist = world > 1 or (os.environ.get("HYPEL_DP_SELFTEST") == "1" and "RANK" in os.environ)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend_name == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend_name)

    from hypelcnn_amd.backend import HipBackend, note_collective
    be = HipBackend()
    classifier = args.workload in CLASSIFIER_WORKLOADS
    if classifier:
        name, cfg, patch, chans, classes, dflt, mac = CLASSIFIER_WORKLOADS[args.workload]
        nb = args.batch or dflt
        ctx, train_step, lr, alg = build_model(nb, be, args.workload)
        ctx.seed = 1234
        ctx.capture_graphs = not args.no_graph
        sess = ctx.session()  # broadcasts rank-0 weights when world > 1
        gen = torch.Generator(device="cpu")
        gen.manual_seed(1234 + rank)
        x = torch.rand((nb, patch, patch, chans), generator=gen).cuda()
        lab = torch.randint(0, classes, (nb,), generator=gen)
        onehot = torch.nn.functional.one_hot(lab, classes).float().cuda()
        ct = train_step.compiled(nb)
        ct.set_input("x", x)
        ct.set_input("labels", onehot)

        def one_step():
            sess.train_step_exchange(ct)  # forward + backward (+ overlapped RCCL gradient all-reduce when N > 1)
            sess.adam_step(lr.eval(sess.global_step))

        loss_fn = ct.loss_value
    else:
        nb, bands, kind, one_step, loss_fn, gan_ops = run_gan_workload(args, be, world, rank)

    for _ in range(args.warmup):
        one_step()
    # the shader clock needs 30-40 ms of uninterrupted work to ramp: pre-warm at least 50 ms of steps
    # whatever --warmup says (untimed, like the W warm-up steps)
    torch.cuda.synchronize()
    if args.dump_outputs:
        n_prewarm = DUMP_PREWARM_STEPS[args.workload]
        for _ in range(n_prewarm):
            one_step()
    else:
        n_prewarm = prewarm_by_time(one_step, use_dist, note_collective)
    if use_dist:
        note_collective()
        dist.barrier()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(args.steps):
        one_step()
        evs[i + 1].record()
    torch.cuda.synchronize()
    if use_dist:
        note_collective()
        dist.barrier()
    dt = time.perf_counter() - t0
    step_ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps))
    dumped = None
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step, read before anything else runs a step
        if classifier:
            outs = {"loss": np.float64([ct.loss_value()]),
                    "logits": ct.value(train_step.loss.per_sample.logits).cpu().numpy()}
            step_sess = sess
        else:
            outs = {"loss_" + k.replace("/", "_"): np.float64([v]) for k, v in gan_ops.losses().items()}
            step_sess = gan_ops.ctx.session()
        outs["params"] = step_sess.params.cpu().numpy()
        outs["gradients"] = step_sess.grads.cpu().numpy()
        dumped = dump_outputs(args.dump_outputs, outs)
    median_ms = step_ms[len(step_ms) // 2]
    if use_dist:
        t = torch.tensor([dt], device="cuda")
        note_collective()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t[0])
    loss = loss_fn()
    assert np.isfinite(loss), "non-finite loss"
    # From here to the result line everything is --full only: a plain run goes straight to the line.
    # Shader clock / power of this rank's GPU: sampled over an UNTIMED replay of the same steps behind the timed region, never
    # inside it -- a host thread that reads sysfs (every read is a query to the GPU's power firmware) every 4 ms cost the
    # launch-bound CycleGAN step 15 %, CUT 1.3 % and the headline 0.6 % when it ran under the timer (round 6, NOTES 6.L).
    if args.full:
        clock = ClockSampler(torch.cuda.current_device())  # (the device this rank actually runs on, not LOCAL_RANK: ranks may share one)
        if classifier and not use_dist:
            n_clock = max(3, min(200, int(0.5 / max(dt / args.steps, 1e-6)) + 1))
            with clock:
                for _ in range(n_clock):
                    one_step()
                torch.cuda.synchronize()
    in_sync = None
    if args.full and use_dist and classifier:
        # data-parallel invariant: every rank holds bit-identical weights after the same all-reduced updates
        digest = torch.stack([sess.params.double().sum(), sess.params.double().abs().max()])
        lo, hi = digest.clone(), digest.clone()
        note_collective()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        note_collective()
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        in_sync = bool(torch.equal(lo, hi))

    pipeline = None
    if args.full and classifier and args.workload == "hypelcnn" and not args.no_input_pipeline:
        # second, clearly labelled measurement: the same step fed by the device-side input pipeline (row a10 of the
        # scope table): BatchIterator over a resident pool + fused gather/augmentation kernel inside every step
        it = input_pipeline_iterator(be, nb, patch, chans, classes, rank)

        def piped_step():
            xb, ob, _ = it.next_batch()
            ct.set_input("x", xb)
            ct.set_input("labels", ob)
            sess.train_step_exchange(ct)
            sess.adam_step(lr.eval(sess.global_step))

        for _ in range(5):
            piped_step()
        if use_dist:
            note_collective()
            dist.barrier()
        torch.cuda.synchronize()
        tp = time.perf_counter()
        n_p = min(args.steps, 50)
        for _ in range(n_p):
            piped_step()
        torch.cuda.synchronize()
        if use_dist:
            note_collective()
            dist.barrier()
        dtp = time.perf_counter() - tp
        if use_dist:
            t = torch.tensor([dtp], device="cuda")
            note_collective()
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dtp = float(t[0])
        pipeline = {"what": "same train step with the device input pipeline in the loop: epoch permutation over a "
                            "resident pool of 8192 patches, rot90 / flips / spectral shift drawn per sample on the "
                            "device, one fused hypel_augment_patches_f32 gather+augment launch per step",
                    "steps": n_p, "ms_per_step": dtp / n_p * 1e3, "value": nb * world * n_p / dtp, "unit": "patches/s"}

    roof = None
    cpu = None
    if args.full and rank == 0 and classifier:
        ev_steps = max(2, min(5, args.steps))
        ms, flops, n_launch = measure_gemm_events(ct, sess, lr, ev_steps)
        achieved = flops / (ms * 1e-3) / 1e12
        traffic, traffic_source = pmc_traffic(args.workload, nb, n_launch // ev_steps)
        share = measure_gemm_events.split_flop_share
        split_on = share > 0
        # The launches of a step run on two matrix pipes: the split-operand kernels (six bf16 MFMAs per fp32 step) and, for
        # narrow / small / n <= 16 products, the fp32 MFMA kernels.  `peak` is the peak of the kernels that do the bulk of the
        # FLOP (the split kernels' fp32-equivalent 2.5 PF / 6 when they are on); `frac_vs_fp32_mfma` prices the same
        # achieved rate against the fp32 matrix peak, the yardstick of rounds 1-4.
        peak = PEAK_SPLIT6_TFLOPS if split_on else PEAK_F32_MFMA_TFLOPS
        roof = {"bound": "mfma",
                "kernel": ("hypel_seg_gemm_f32 / hypel_seg_gemm_multi_f32 with HYPEL_GEMM_SPLIT6 (3 x bf16 split operands, "
                           "six v_mfma_f32_32x32x16_bf16 per step, fp32 accumulate) for %.0f %% of the FLOP; the rest on the "
                           "fp32 MFMA kernels (v_mfma_f32_32x32x2, 16x16x4 for n <= 16)" % (100 * share)) if split_on else
                          "hypel_seg_gemm_f32 / hypel_seg_gemm_multi_f32 (fp32 MFMA: v_mfma_f32_32x32x2, 16x16x4 for n <= 16)",
                "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                "peak_note": ("fp32-equivalent: dense bf16 MFMA peak 2500 TFLOP/s (at 2.4 GHz) / 6 partial products; the split kernels "
                              "run against the 1.4 kW power cap at 1.4-1.8 GHz inside a launch (profiles/r5_exp_split_ablation.txt; "
                              "sustained_clock_ghz = this run's average over an untimed replay of the step loop)") if split_on
                             else "fp32 MFMA peak",
                "frac_vs_fp32_mfma": achieved / PEAK_F32_MFMA_TFLOPS, "peak_fp32_mfma": PEAK_F32_MFMA_TFLOPS,
                "split6_flop_share": share, "split6_launches_per_step": measure_gemm_events.split_launches,
                "traffic": traffic, "traffic_source": traffic_source, "launches_per_step": n_launch // ev_steps,
                "avg_launch_us": ms * 1e3 / n_launch,
                "gemm_ms_per_step": ms / ev_steps,
                "algorithmic_gflop_per_step": flops / ev_steps / 1e9,
                "algorithmic_bytes_per_launch": measure_gemm_events.bytes_per_launch,
                "kernel_launches_per_step": len(ct.serial_launches()) + 1}  # every launch of the step + the optimiser
        roof.update(clock.summary())
        busy, busy_source = pmc_mfma_busy(args.workload)
        if busy is not None:
            # NOT measured by this run: the matrix-pipe busy share of the committed SQ-counter pass of the same command
            roof["committed_profiles"] = {"mfma_busy_pmc": busy["busy"], "mfma_useful_pmc": busy["useful"], "source": busy_source}
        if world == 1 and not args.no_cpu_baseline:
            cpu = cpu_baseline(workload=args.workload)
    if args.full and rank == 0 and not classifier:
        step_ms_mean = dt / args.steps * 1e3
        gen_ms, gen_flops, n_gen, n_launch = measure_gan_events(gan_ops, nb, bands, max(2, min(5, args.steps)))
        boundary_us = 1.7  # MI355X_MICROARCH.md price list, "boundary": 1.45-1.9 us per dependent kernel boundary
        launch_floor_ms = n_launch * boundary_us * 1e-3
        if bands > 128:
            # GAN half of cfg5 (B = 360): the generator is fp32 matrix-core work (gan_mfma.hip) -- its exact-tap FLOP over
            # its kernel time against the fp32 MFMA peak
            achieved = gen_flops / (gen_ms * 1e-3) / 1e12
            roof = {"bound": "mfma", "kernel": "gan_generator_{fwd,bwd}_mfma_kernel (v_mfma_f32_16x16x4_f32)",
                    "achieved": achieved, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                    "frac": achieved / PEAK_F32_MFMA_TFLOPS, "traffic": None,
                    "generator_launches_per_step": n_gen, "generator_ms_per_step": gen_ms,
                    "generator_share_of_step": gen_ms / step_ms_mean,
                    "algorithmic_gflop_per_step": gen_flops / 1e9,
                    "flop_convention": "exact taps; forward 2 FLOP per MAC, backward 4 (data + filter gradient; no "
                                       "recompute is counted)",
                    "launches_per_step": n_launch, "launch_floor_ms": launch_floor_ms}
        else:
            # cfg4 (B = 64): 12 k multiply-adds per sample and generator pass -- neither HBM nor the matrix cores bound
            # the step, its kernel boundaries do.  HBM line for the record (algorithmic bytes: x and y read once,
            # SURVEY 8d), and the launch floor = launches x the guide's per-boundary cost against the measured step.
            # the step is a chain of dependent launches: the bound that means something is the sum of the per-launch floors
            # (guide: 1.45-1.9 us per dependent kernel boundary), not HBM (x and y once = 1 MB against 8 TB/s: 0.06 %)
            alg_bytes = 2 * 4 * bands * nb
            roof = {"bound": "launch-latency chain", "kernel": "gan phases (fused generator / dense-stack / loss launches)",
                    "achieved": launch_floor_ms, "peak": step_ms_mean, "unit": "ms (sum of per-launch floors vs measured step)",
                    "frac": launch_floor_ms / step_ms_mean, "traffic": None,
                    "note": "frac = launches x boundary cost / step: what share of the step the dependent-launch floor explains",
                    "launches_per_step": n_launch, "boundary_us": boundary_us, "launch_floor_ms": launch_floor_ms,
                    "hbm_gbps_for_the_record": alg_bytes / (dt / args.steps) / 1e9,
                    "generator_launches_per_step": n_gen, "generator_ms_per_step": gen_ms}
        if world == 1 and not args.no_cpu_baseline:
            cpu = gan_cpu_baseline(kind, bands)
    if use_dist:
        note_collective()
        dist.barrier()
    if rank == 0:
        if classifier:
            metric = {"hypelcnn": baseline_metric(),
                      "dualcnn": "HSI+LiDAR patches/sec fwd+bwd (GRSS2018 11x11x49, DUALCNN)"}[args.workload]
            cfg_d = {"workload": {"hypelcnn": "BASELINE.json configs[1]: GRSS2013 HYPELCNNModel, batch 1024 per GPU, "
                                              "fp32 HIP kernels; train step (fwd+bwd+TF1-Adam), 7x7 patch, 144 HSI + 1 "
                                              "LiDAR bands, 15 classes, alg_param_hypelcnn.json, random-init weights",
                                  "dualcnn": "GRSS2018 DUALCNNModel train step (fwd+bwd+TF1-Adam), 11x11 patch, 48 "
                                             "HSI + 1 LiDAR bands, 20 classes, alg_param_dualcnn.json, random-init "
                                             "weights"}[args.workload],
                     "batch_per_gpu": nb, "global_batch": nb * world,
                     "parallelism": f"dp{world}" if world > 1 else "single",
                     "hip_graph": ctx.capture_graphs, "loss": loss}
            if in_sync is not None:
                cfg_d["dp_weights_identical_across_ranks"] = in_sync
            if use_dist:
                cfg_d["communicator"] = {"backend": dist.get_backend(), "ranks": dist.get_world_size()}
            if world > 1:
                cfg_d["batch_norm"] = "synchronised (global batch)" if args.sync_bn else "per rank"
            if mac:
                cfg_d["mfma_ceiling_patches_per_s_per_gpu"] = PEAK_F32_MFMA_TFLOPS * 1e12 / (6 * mac)
                cfg_d["split6_ceiling_patches_per_s_per_gpu"] = PEAK_SPLIT6_TFLOPS * 1e12 / (6 * mac)
            unit = "patches/s"
        else:
            metric = f"spectral pairs/sec, full {kind} train step (all sequential train ops + Adam)"
            cfg_d = {"workload": f"{kind} on [{nb},1,1,{bands}] synthetic pairs (y = x / ratio), reference "
                                 "hyper-parameters (gan_train_for_shadow.py:44-49), zero-init generators",
                     "batch_per_gpu": nb, "global_batch": nb * world,
                     "parallelism": f"dp{world}" if world > 1 else "single", "hip_graph": not args.no_graph,
                     "loss": loss, "steps_per_s": args.steps / dt}
            unit = "pairs/s"
        out = {"metric": metric, "value": nb * world * args.steps / dt,
               "unit": unit, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": dt / args.steps * 1e3, "ms_per_step_median": median_ms,
               "ms_per_step_p10_p90": [step_ms[len(step_ms) // 10], step_ms[(9 * len(step_ms)) // 10]],
               "prewarm_steps": n_prewarm, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": ("f32 (3 x bf16 split operands, 6 partial products, fp32 accumulate)"
                         if classifier and split6_flop_share(ct)[0] else "f32"),
               "data": "synthetic", "config": cfg_d, "roofline": roof, "cpu_baseline": cpu}
        if pipeline is not None:
            out["with_input_pipeline"] = pipeline
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        out["commit"], note = commit_label()
        if note:
            out["commit_note"] = note
        print(json.dumps(out))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
