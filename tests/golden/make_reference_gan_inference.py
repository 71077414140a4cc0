#!/usr/bin/env python3
"""Pin the two GAN INFERENCE programs by executing the reference's own text (build container only; needs /root/reference).

`gan/gan_infer_image_for_shadow.py::main` and `gan/gan_infer_for_shadow.py::main` run UNCHANGED; what they reach outside
themselves is replaced by stand-ins defined here:

  * a small loader (9 x 11 pixels, 5 or 7 bands, float32 or uint16, a 0/1 shadow map, seeded) whose data set is the
    reference's own `BasicDataSet` and whose shadow ratio is the reference's `calculate_shadow_ratio`;
  * `tf.compat.v1.Session` whose `run` evaluates what it is asked for: the conversion's generator output is a SCRIPTED
    per-pixel function g(x) = tanh(1.7 x - 0.4 + 0.01 b) (float32) whose every fed pixel is recorded; the scoring
    statistic (`create_stats_tensor`, gan/wrappers/gan_common.py:315-330, unchanged) is evaluated in float32 NumPy
    through lazy stand-ins for the dozen `tf.*` ops it uses;
  * the inference wrappers' graph builders (`construct_inference_graph` -> g, the placeholders) and restorers
    (recorded calls); the hooks themselves (`create_inference_hook`, `create_base_validation_hook`, `ValidationHook`,
    `PeerValidationHook`, `BestRatioHolder`, `load_samples_for_testing`) are the reference's;
  * recording `tifffile.imwrite`, `tqdm`, `get_rgb_from_hsi` (returns zeros), the summary writer and the band-ratio
    plot; Python's `random` seeded.

Written to tests/golden/reference_gan_inference.json / .npz: per conversion case the fed pixels in order, the restore
call, the generator direction, the written file names, the raster (dtype and values); per scoring case the sampled
(x, y) points, the divergences and the best_ratio JSON files; and one scripted BestRatioHolder sequence.  Only data is
written."""
import contextlib
import importlib
import json
import os
import random
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


def g(x):
    x = np.asarray(x, np.float32)
    b = np.arange(x.shape[-1], dtype=np.float32)
    return np.tanh(np.float32(1.7) * x - np.float32(0.4) + np.float32(0.01) * b).astype(np.float32)


def scene(bands, dtype, seed):
    rng = np.random.default_rng(seed)
    h, w = 9, 11
    casi = rng.random((h, w, bands)) * 3000 + 400
    smap = (rng.random((h, w)) < 0.35).astype(np.uint8)
    casi = np.where(smap[..., None] == 1, casi * 0.45, casi)
    casi = np.rint(casi).astype(dtype) if dtype == "uint16" else casi.astype(np.float32)
    return casi, smap


# ------------------------------------------------------------------------------------------------ lazy float32 tensors
class Lazy:
    def __init__(self, fn):
        self.fn = fn

    def ev(self, feed):
        return self.fn(feed)

    def _bin(self, other, op, rev=False):
        def f(feed):
            a, b = self.ev(feed), ev(other, feed)
            return op(b, a) if rev else op(a, b)
        return Lazy(f)

    __truediv__ = lambda s, o: s._bin(o, np.divide)
    __mul__ = lambda s, o: s._bin(o, np.multiply)
    __rmul__ = lambda s, o: s._bin(o, np.multiply, True)
    __add__ = lambda s, o: s._bin(o, np.add)
    __radd__ = lambda s, o: s._bin(o, np.add, True)
    __sub__ = lambda s, o: s._bin(o, np.subtract)
    __rsub__ = lambda s, o: s._bin(o, np.subtract, True)

    def __getitem__(self, mask):
        return Lazy(lambda feed: self.ev(feed)[ev(mask, feed)])


def ev(v, feed):
    if isinstance(v, Lazy):
        return v.ev(feed)
    return v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v


def lazy(fn):
    return lambda *a, **k: Lazy(lambda feed: fn(*[ev(x, feed) for x in a], **{n: ev(x, feed) for n, x in k.items()}))


def placeholder(name):
    p = Lazy(lambda feed: np.asarray(feed[name], np.float32))
    p.name = name
    return p


def lazy_tf():
    f32 = lambda v: np.asarray(v, np.float32)  # noqa: E731
    v1 = types.SimpleNamespace(
        where=lazy(lambda c, a, b: f32(np.where(c, a, b))),
        placeholder=lambda dtype=None, shape=None, name=None: placeholder(name),
        train=types.SimpleNamespace(get_global_step=lambda: None),
        disable_v2_behavior=lambda: None, Session=Session)
    return types.SimpleNamespace(
        compat=types.SimpleNamespace(v1=v1), float32=np.float32,
        squeeze=lazy(lambda x, axis: np.squeeze(x, axis=tuple(axis))),
        reduce_all=lazy(lambda input_tensor, axis: np.all(input_tensor, axis=axis)),
        math=types.SimpleNamespace(is_finite=lazy(np.isfinite), log=lazy(lambda x: f32(np.log(x)))),
        not_equal=lazy(lambda a, b: a != b), zeros_like=lazy(np.zeros_like), abs=lazy(np.abs))


def reduce_mean(x, axis=None):
    return Lazy(lambda feed: np.mean(ev(x, feed), axis=axis, dtype=np.float32))


def reduce_sum(x, axis=None):
    return Lazy(lambda feed: np.sum(ev(x, feed), axis=axis, dtype=np.float32))


def reduce_std(x, axis=None):
    return Lazy(lambda feed: np.std(ev(x, feed), axis=axis, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ session, loader, wrappers
LOG = {}


class Session:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def run(self, fetches, feed_dict=None):
        if fetches == "G(x)":  # the conversion: one pixel [1, 1, 1, B]
            (x,) = feed_dict.values()
            LOG["fed"].append(np.asarray(x, np.float32).reshape(-1).copy())
            LOG["fed_at"].append(LOG["points"][-1])
            return g(x)
        feed = {k.name: v for k, v in feed_dict.items()}
        if isinstance(fetches, list):
            return [ev(f, feed) for f in fetches]
        return ev(fetches, feed)


class Restorer:
    def restore(self, sess, path):
        LOG["restored"].append(path)


class Loader:
    def __init__(self, path, ref_ops):
        bands, dtype, seed = path.split(":")
        self.casi, self.smap = scene(int(bands), dtype, int(seed))
        self.ref_ops = ref_ops

    def load_data(self, neighborhood, normalize):
        ds = self.ref_ops.BasicDataSet(shadow_creator_dict=None, casi=self.casi, lidar=None, neighborhood=neighborhood,
                                       normalize=normalize)
        real = ds.get_data_point

        def get_data_point(x, y):
            LOG["points"].append([int(x), int(y)])
            return real(x, y)
        ds.get_data_point = get_data_point
        return ds

    def load_shadow_map(self, neighborhood, data_set):
        shadow_map = np.pad(self.smap, neighborhood, mode="symmetric")
        return shadow_map, self.ref_ops.calculate_shadow_ratio(data_set.casi, shadow_map,
                                                               np.logical_not(shadow_map).astype(int))

    def get_band_measurements(self):
        return np.linspace(400, 1000, self.casi.shape[2])


def stub_wrappers(registry, cyc_mod, gan_mod):
    """The reference's inference wrappers with their graph builders replaced: construct_inference_graph -> g on the
    placeholder, make_inference_graph -> the tokens the Session knows, restorers recorded."""
    d = registry.get_infer_wrapper_dict()
    for w in d.values():
        w.construct_inference_graph = lambda inp, is_shadow, clip_invalid_values: Lazy(lambda feed: g(inp.ev(feed)))

        def make(data_set, is_shadow_graph, clip_invalid_values):
            LOG["direction"].append("x2y" if is_shadow_graph else "y2x")
            return "x", "G(x)"
        w.make_inference_graph = make
        w.create_generator_restorer = lambda: Restorer()
    cyc_mod.tf = lazy_tf()
    gan_mod.create_input_tensor = lambda data_set, is_shadow_graph: placeholder("x" if is_shadow_graph else "y")
    return d


def main():
    S.install()
    import tfgan_standin as TG
    TG.install()
    written = []
    sys.modules["common.hsi_rgb_converter"] = types.SimpleNamespace(
        get_rgb_from_hsi=lambda bands, img: np.zeros(img.shape[:2] + (3,)))
    sys.modules["tifffile"] = types.SimpleNamespace(imread=None, imwrite=None)
    ref_ops = importlib.import_module("common.common_nn_ops")
    registry = importlib.import_module("gan.wrapper_registry")
    cyc_mod = importlib.import_module("gan.wrappers.cycle_gan_wrapper")
    gan_mod = importlib.import_module("gan.wrappers.gan_wrapper")
    gc = importlib.import_module("gan.wrappers.gan_common")
    img_prog = importlib.import_module("gan.gan_infer_image_for_shadow")
    score_prog = importlib.import_module("gan.gan_infer_for_shadow")

    gc.tf, gc.reduce_mean, gc.reduce_sum, gc.reduce_std = lazy_tf(), reduce_mean, reduce_sum, reduce_std
    gc.scalar = lambda name, tensor, collections=None: Lazy(lambda feed: name)
    gc.summary_io = types.SimpleNamespace(SummaryWriterCache=types.SimpleNamespace(
        get=lambda d: (os.makedirs(d, exist_ok=True), types.SimpleNamespace(add_summary=lambda s, i: None))[1]))
    gc.plot_overall_info = lambda *a, **k: None
    for prog in (img_prog, score_prog):
        prog.tf = lazy_tf()
        prog.set_all_gpu_config = lambda: None
        prog.get_loader_from_name = lambda name, path: Loader(path, ref_ops)
        prog.get_infer_wrapper_dict = lambda: stub_wrappers(registry, cyc_mod, gan_mod)
    img_prog.imwrite = lambda path, data, **kw: written.append((os.path.basename(path), np.array(data), kw))
    img_prog.tqdm = lambda total=None: types.SimpleNamespace(update=lambda n: None, close=lambda: None)
    score_prog.SessionRunContext = lambda original_args, session: types.SimpleNamespace(session=session)

    meta, arrays = {"convert": {}, "score": {}}, {}
    tmp = tempfile.mkdtemp()
    for bands, dtype, seed in ((5, "float32", 1), (7, "uint16", 2)):
        path = f"{bands}:{dtype}:{seed}"
        casi, smap = scene(bands, dtype, seed)
        arrays[f"scene/{path}/casi"], arrays[f"scene/{path}/shadow_map"] = casi, smap
        for mode in ("shadow", "deshadow", "none", ""):
            for conv_all in ("false", "true"):
                LOG.update(fed=[], fed_at=[], restored=[], direction=[], points=[])
                written.clear()
                sys.argv = ["prog", "--loader_name", "Stub", "--path", path, "--base_log_path", "/ckpt/model.ckpt-4200",
                            "--output_path", "/out", "--make_them_shadow", mode, "--convert_all", conv_all,
                            "--gan_type", "cycle_gan"]
                with contextlib.redirect_stdout(open(os.devnull, "w")):
                    img_prog.main(None)
                key = f"{path}/{mode or 'empty'}/{conv_all}"
                fed_idx = [int(y * 11 + x) for x, y in LOG["fed_at"]]  # the pixel each sess.run converted
                fed = np.asarray(LOG["fed"], np.float32).reshape(-1, bands)
                meta["convert"][key] = {"restored": LOG["restored"], "direction": LOG["direction"],
                                        "files": [w[0] for w in written], "imwrite_kwargs": [w[2] for w in written],
                                        "dtype": str(written[0][1].dtype), "n_fed": int(fed.shape[0])}
                arrays[f"convert/{key}/raster"] = written[0][1]
                arrays[f"convert/{key}/fed"] = fed
                arrays[f"convert/{key}/fed_pixels"] = np.asarray(fed_idx, np.int64)
        for gan_type in ("cycle_gan", "gan_x2y", "gan_y2x"):
            random.seed(1000 + seed)
            LOG.update(fed=[], fed_at=[], restored=[], direction=[], points=[])
            log_dir = os.path.join(tmp, f"{gan_type}_{path.replace(':', '_')}")
            sys.argv = ["prog", "--loader_name", "Stub", "--path", path, "--base_log_path", log_dir,
                        "--number_of_samples", "40", "--gan_type", gan_type]
            with contextlib.redirect_stdout(open(os.devnull, "w")):
                score_prog.main(None)
            key = f"{path}/{gan_type}"
            files = {f: json.load(open(os.path.join(log_dir, f))) for f in sorted(os.listdir(log_dir))}
            meta["score"][key] = {"restored": [os.path.basename(p) for p in LOG["restored"]], "best_ratio": files}
            arrays[f"score/{key}/points"] = np.asarray(LOG["points"], np.int64)
    shutil.rmtree(tmp)

    holder, other = gc.BestRatioHolder(4), gc.BestRatioHolder(4)
    seq = [(10, 0.5), (20, 0.25), (30, 0.5), (40, 0.75), (50, 0.125), (60, 0.25), (70, 1.5)]
    for it, d in seq:
        holder.add_point(np.int64(it), np.float64(d))
    seq2 = [(20, 0.3), (50, 0.6), (80, 0.0), (30, 0.9)]
    for it, d in seq2:
        other.add_point(it, d)
    meta["best_ratio_holder"] = {"max_size": 4, "sequence": seq, "holder": holder.data_holder, "sequence_2": seq2,
                                 "holder_2": other.data_holder,
                                 "common": gc.BestRatioHolder.create_common_iterations(holder, other).data_holder,
                                 "json": json.dumps(holder.data_holder)}
    with open(os.path.join(HERE, "reference_gan_inference.json"), "w") as f:
        json.dump(meta, f, sort_keys=True, indent=0, separators=(",", ":"))
    np.savez_compressed(os.path.join(HERE, "reference_gan_inference.npz"), **arrays)
    print("wrote reference_gan_inference.json / .npz:", len(meta["convert"]), "conversions,", len(meta["score"]),
          "scorings")


if __name__ == "__main__":
    main()
