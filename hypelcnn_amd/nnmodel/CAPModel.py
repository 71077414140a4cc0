"""Capsule classifier on the MI355X graph builder (reference nnmodel/CAPModel.py:30-159, modelconfigs/alg_param_capn.json).

Conv1 (k1 x k1, VALID, batch norm, ReLU) -> PrimaryCaps (k2 x k2, VALID, batch norm, ReLU), viewed as I = pixels x
`primary_capsule_count` capsules of width D -> one [D, J*D] map per capsule -> `iter_routing` rounds of dynamic routing ->
y_conv = length of the class vectors.  Training with `enable_decoding` adds the label-masked decoder (fc 512, fc 1024 with
leaky ReLU, fc patch-size sigmoid) and its reconstruction error to the loss.  Both capsule widths come from
`digit_capsule_output_space`, as in the reference (its `primary_capsule_output_space` key is never read).

Three behaviours of the reference that are kept on purpose:
  * the batch norms always normalise with the statistics of the batch in hand (tf_slim's default is_training=True is never
    overridden), in evaluation towers too; only the training step moves the moving averages;
  * the routing logits are summed over the batch, so the logits of a sample depend on which samples share its launch:
    whole-scene inference in chunks depends on the chunk size, exactly as the reference's does on its batch size;
  * the loss is the public `get_loss_func`: softmax cross-entropy on y_conv (+ mean squared reconstruction error); the
    margin loss of the reference is name-mangled dead code and is not built.

Single device only: a data-parallel run would need an all-reduce of the agreement inside every routing iteration.
"""
import os

from hypelcnn_amd import graph as g
from hypelcnn_amd.common.common_nn_ops import ModelOutputTensors
from hypelcnn_amd.nnmodel.NNModel import NNModel


def _world_size():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size()
    except ImportError:
        pass
    return int(os.environ.get("WORLD_SIZE", "1"))


class CAPModel(NNModel):

    def create_tensor_graph(self, model_input_params, class_count, algorithm_params):
        if _world_size() > 1:
            raise NotImplementedError(
                "CAPModel does not run data parallel (WORLD_SIZE > 1): its routing agreement is summed over the batch, so "
                "every routing iteration would need an all-reduce to stay equal to one device")
        p = algorithm_params
        training = model_input_params.is_training
        x = model_input_params.x
        width = p["digit_capsule_output_space"]
        count = p["primary_capsule_count"]
        bn = dict(normalizer_fn=g.batch_norm, normalizer_params={"is_training": True, "update_moving": training})
        net = g.conv2d(x, p["feature_count"], [p["conv_layer_kernel_size"]] * 2, scope="Conv1_layer", padding="VALID", **bn)
        net = g.conv2d(net, count * width, [p["primary_caps_kernel_size"]] * 2, scope="PrimaryCaps_layer",
                       padding="VALID", **bn)
        with g.variable_scope("DigitCaps_layer"):
            y_conv, v = g.capsule_routing(net, count, class_count, width, p["iter_routing"])
            decoded = None
            if training and p["enable_decoding"]:
                labels = model_input_params.y
                if hasattr(labels, "bind"):
                    labels = labels.bind(x.tower)
                lrelu = g.leaky_relu(p["lrelu_alpha"])
                with g.variable_scope("Decoder"):
                    net = g.label_mask(v, labels, class_count, width)
                    net = g.fully_connected(net, 512, scope="fc1", activation_fn=lrelu)
                    net = g.fully_connected(net, 1024, scope="fc2", activation_fn=lrelu)
                    decoded = g.fully_connected(net, x.npix * x.c, scope="fc3", activation_fn=g.sigmoid)
        return ModelOutputTensors(y_conv=y_conv, image_output=decoded, image_original=x, histogram_tensors=[])

    def get_loss_func(self, tensor_output, label):
        loss = g.softmax_cross_entropy_with_logits(labels=label, logits=tensor_output.y_conv)
        if tensor_output.image_output is not None:
            loss = loss + g.mean_squared_reconstruction(tensor_output.image_output, tensor_output.image_original)
        return loss
