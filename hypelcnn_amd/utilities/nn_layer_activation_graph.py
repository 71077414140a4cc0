"""Histograms of the tapped layer activations of a trained model (reference utilities/nn_layer_activation_graph.py):

    python -m hypelcnn_amd.utilities.nn_layer_activation_graph --loader_name <loader> --path <dir> --neighborhood <n>
        --model_name HYPELCNNModel --algorithm_param_path <json> --base_log_path <checkpoint | directory>
        --output_path <dir> [--batch_size 20] [--domain controlled|sample|all] [--base_bins 480]

The inference tower is restored from a checkpoint and fed; every tensor the model taps (ModelOutputTensors.
histogram_tensors -- HYPELCNN's spectral_expansion, spectral_reduction, spatial and classification) gets one histogram
of uniform bins between its global minimum and maximum, int(base_bins / size_0 * size_i) of them for a tap of size_i
elements per sample, averaged over the batches.  The activations never leave the device (common/device_activation.py):
a first pass folds the ranges, a second one the histograms.

--domain controlled (default) is the reference's input: every sample all zeros with the last (LiDAR) channel ones.  The
samples are identical and inference is deterministic, so ONE batch of --batch_size samples is the reference's mean over
the batches it collects, and one forward serves both passes.  --domain sample (the loader's samples) and --domain all
(every pixel of the scene) are cut from the resident scene as infer_for_classification does, in two passes over the
batches; the last batch may be partial, and the mean is counts / batches like the reference's numpy.mean(all_hists).

Departures from the reference: it parses the flags it uses; a tap whose bin count rounds to 0 gets 1 bin;
a tap that needs more than HYPEL_ACT_MAX_BINS bins is refused by name; a single device only.  Writes <tap>_hist.json
(name, bins, lo, hi, counts, mean, batches, finite, nonfinite, outside) and, where matplotlib can be imported, the
reference's <tap>_fig.jpg."""
import argparse
import json
import os
import time

import numpy
import torch

from hypelcnn_amd.classify.infer_for_classification import create_all_scene_data, create_sample_data
from hypelcnn_amd.classify.monitored_session_runner import latest_checkpoint, restore_checkpoint
from hypelcnn_amd.common.cmd_parser import add_parse_cmds_for_loaders, add_parse_cmds_for_loggers, \
    add_parse_cmds_for_models, add_parse_cmds_for_trainers
from hypelcnn_amd.common.common_nn_ops import GraphContext, ModelInputParams, NNParams, Template, _capture_forward, \
    get_model_from_name, simple_nn_iterator
from hypelcnn_amd.common.device_activation import ActivationTaps, tap_bins
from hypelcnn_amd.importer.GeneratorImporter import GeneratorImporter

DOMAINS = ("controlled", "sample", "all")


def build_parser():
    parser = argparse.ArgumentParser()
    add_parse_cmds_for_loaders(parser)
    add_parse_cmds_for_loggers(parser)
    add_parse_cmds_for_models(parser)
    add_parse_cmds_for_trainers(parser)
    parser.add_argument("--domain", nargs="?", type=str, default="controlled",
                        help="controlled (zeros with the last channel ones, the reference's input), sample (the "
                             "loader's samples) or all (every pixel of the scene)")
    parser.add_argument("--base_bins", nargs="?", type=int, default=480, help="Bins of the first tap's histogram")
    return parser


class TapRun:
    """The restored inference tower of a run and its input batches."""

    def __init__(self, flags, backend=None):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError("nn_layer_activation_graph runs on a single device")
        if flags.domain not in DOMAINS:
            raise ValueError(f"Domain flags does not support value:{flags.domain}")
        if flags.algorithm_param_path is None:
            raise IOError("Algorithm parameter file is not given")
        self.flags = flags
        self.importer = GeneratorImporter()
        training, test, validation, _, class_range, scene_shape, _ = self.importer.read_data_set(
            flags.loader_name, flags.path, 0.1, 0, flags.neighborhood, True)
        self.data_shape = tuple(int(v) for v in validation.dataset.get_data_shape())
        if flags.domain == "all":
            validation = create_all_scene_data(scene_shape, validation)
        elif flags.domain == "sample":
            validation = create_sample_data(training, test, validation)
        algorithm_params = json.load(open(flags.algorithm_param_path, "r"))
        algorithm_params["batch_size"] = flags.batch_size
        nn_model = get_model_from_name(flags.model_name)
        _, _, self.tensor = self.importer.convert_data_to_tensor(test, training, validation, class_range)
        template = Template("nn_core", nn_model.create_tensor_graph, class_count=class_range.stop)
        ctx = GraphContext(template, backend)
        iterator = simple_nn_iterator(self.tensor.dataset, flags.batch_size)
        images, _ = iterator.get_next()
        self.outputs = template(ModelInputParams(x=images, y=None, device_id="/gpu:0", is_training=False),
                                algorithm_params=algorithm_params)
        self.taps = [(pair.tensor, pair.name) for pair in self.outputs.histogram_tensors]
        if not self.taps:
            raise ValueError(f"{flags.model_name} taps no activations (its histogram_tensors is empty)")
        self.nn_params = NNParams(input_iterator=iterator, data_with_labels=validation, metrics=None,
                                  predict_tensor=self.outputs.y_conv)
        self.session = ctx.session()
        ckpt = flags.base_log_path
        if os.path.isdir(ckpt):
            ckpt = latest_checkpoint(ckpt)
        if ckpt is None or not os.path.exists(ckpt):
            raise IOError(f"No checkpoint found at {flags.base_log_path}")
        restore_checkpoint(self.session, ckpt)

    def controlled_batch(self):
        """reference ControlledDataImporter: zeros, the last channel ones, --batch_size identical samples"""
        x = numpy.zeros((self.flags.batch_size,) + self.data_shape, numpy.float32)
        x[..., -1] = 1.0
        return torch.from_numpy(x).to(self.session.backend.device)

    def batches(self):
        """the input batches of one pass, in order"""
        if self.flags.domain == "controlled":
            yield self.controlled_batch()
            return
        self.importer.init_tensors(self.session, self.tensor, self.nn_params)
        while True:
            batch = self.nn_params.input_iterator.next_batch()
            if batch is None:
                return
            yield batch[0]

    def forward(self, x):
        ct = self.session.compile(self.outputs.tower, int(x.shape[0]))
        _capture_forward(None, self.session, ct)
        ct.set_input("x", x)
        ct.forward()
        return ct


def plot(path, name, edges, mean):
    """the reference's figure -- its plot calls, labels and title -- where matplotlib is installed, drawn on a Figure of
    its own (no pyplot, no global state); -> whether it was written"""
    try:
        from matplotlib.figure import Figure
    except ImportError:
        return False
    fig = Figure()
    ax = fig.add_subplot(1, 1, 1)
    ax.plot(edges[:-1], mean, label=name)
    ax.set_xlim(min(edges), max(edges))
    ax.set_xlabel("Value")
    ax.set_ylabel("Counts")
    ax.fill_between(edges[:-1], mean)
    ax.set_title(name)
    fig.savefig(path)
    return True


def main(argv=None, backend=None):
    flags, _ = build_parser().parse_known_args(argv)
    start_time = time.time()
    run = TapRun(flags, backend)
    acts = ActivationTaps(run.session, run.taps, tap_bins(run.taps, flags.base_bins))
    n_batches, ct = 0, None
    for x in run.batches():
        ct = run.forward(x)
        acts.fold_range(ct)
        n_batches += 1
    if n_batches == 0:
        raise ValueError(f"--domain {flags.domain} yields no batch")
    acts.set_edges()
    if flags.domain == "controlled":
        acts.fold_histogram(ct)  # the one forward still stands in the plan buffers
    else:
        for x in run.batches():
            acts.fold_histogram(run.forward(x))
    os.makedirs(flags.output_path, exist_ok=True)
    records = {}
    for name, r in acts.results().items():
        mean = r["counts"] / n_batches
        records[name] = {"name": name, "bins": int(r["counts"].size), "lo": r["lo"], "hi": r["hi"],
                         "counts": [int(c) for c in r["counts"]], "mean": [float(m) for m in mean],
                         "batches": n_batches, "finite": r["finite"], "nonfinite": r["nonfinite"],
                         "outside": r["outside"]}
        with open(os.path.join(flags.output_path, name + "_hist.json"), "w") as f:
            json.dump(records[name], f)
        plot(os.path.join(flags.output_path, name + "_fig.jpg"), name, r["edges"], mean)
    print("Done evaluation(%.3f sec)" % (time.time() - start_time))
    return records


if __name__ == "__main__":
    main()
