"""Shared GAN machinery (reference gan/wrappers/gan_common.py): scope names, the tfgan-style model records,
the LR schedule, the tensor pool, the phase executor that replaces tfgan's RunTrainOpsHook sequence, and the
band-ratio validation hooks that score a generator (reference :47-219, 315-330, 362-382, 417-429)."""
import collections
import json
import os
from json import JSONDecodeError

import numpy
import torch

from hypelcnn_amd import graph as G

model_generator_name = "Generator"
model_base_name = "Model"
input_x_tensor_name = "x"
input_y_tensor_name = "y"


def adj_shadow_ratio(shadow_ratio, is_shadow):
    return 1. / shadow_ratio if is_shadow else shadow_ratio


class GANModel(collections.namedtuple("GANModel", (
        "tower", "generator_inputs", "generated_data", "generator_scope", "real_data", "discriminator_real_outputs",
        "discriminator_gen_outputs", "discriminator_pool_outputs", "pool_input", "discriminator_scope"))):
    """What tfgan.gan_model returns, plus the discriminator applied to the tensor-pool placeholder."""


CycleGANModel = collections.namedtuple("CycleGANModel", ("model_x2y", "model_y2x", "reconstructed_x",
                                                          "reconstructed_y", "identity_x", "identity_y"))

Phase = collections.namedtuple("Phase", ("name", "terms", "train_groups", "lr_key", "pool"))
GANLoss = collections.namedtuple("GANLoss", ("phases", "tower", "generate_outputs"))


def new_gan_tower(bands):
    """One recorded graph per GAN (TF builds one graph too); variables carry the full TF names (no template prefix)."""
    tower = G.Tower(G.VariableStore(prefix=""), True, name="gan")
    x = tower.placeholder(input_x_tensor_name, None, bands)
    y = tower.placeholder(input_y_tensor_name, None, bands)
    return tower, x, y


def build_gan_model(tower, generator_fn, discriminator_fn, generator_inputs, real_data, pool_name,
                    generator_scope="Generator", discriminator_scope="Discriminator"):
    """tfgan.gan_model: G(inputs), D(G(inputs)), D(real) with shared discriminator variables -- and a third
    application of D on the tensor-pool placeholder (tfgan.gan_loss(tensor_pool_fn=...) re-applies D on pooled data)."""
    with G.variable_scope(generator_scope) as gs:
        generated = generator_fn(generator_inputs)
    with G.variable_scope(discriminator_scope) as ds:
        d_gen = discriminator_fn(generated, generator_inputs)
    with G.variable_scope(discriminator_scope):
        d_real = discriminator_fn(real_data, generator_inputs)
    pool_in = d_pool = None
    if pool_name:
        pool_in = tower.placeholder(pool_name, None, generated.c)
        with G.variable_scope(discriminator_scope):
            d_pool = discriminator_fn(pool_in, generator_inputs)
    return GANModel(tower, generator_inputs, generated, gs, real_data, d_real, d_gen, d_pool, pool_in, ds)


def _get_lr(base_lr, max_number_of_steps):
    """reference :222-244 -- constant for the first half, then polynomial_decay(power=1) to 0."""
    half = max_number_of_steps // 2

    def lr(global_step):
        if global_step < half:
            return base_lr
        decay_steps = max_number_of_steps - half
        s = min(global_step - half, decay_steps)
        return base_lr * (1 - s / decay_steps)

    return lr


class TensorPool:
    """tfgan.features.tensor_pool(pool_size=50, pooling_probability=0.5): until the pool is full the input is
    stored and returned; afterwards with probability 0.5 the input is returned unchanged, otherwise a random pooled
    element is returned and replaced by the input.  One element = one whole batch tensor, as in tfgan."""

    def __init__(self, pool_size=50, pooling_probability=0.5, seed=1234):
        self.pool_size, self.prob = pool_size, pooling_probability
        self.items = []
        self.rng = numpy.random.default_rng(seed)

    def query(self, value):
        if self.pool_size <= 0:
            return value
        if len(self.items) < self.pool_size:
            self.items.append(value.clone())
            return value
        if self.rng.random() >= self.prob:
            return value
        i = int(self.rng.integers(0, len(self.items)))
        out = self.items[i]
        self.items[i] = value.clone()
        return out


class GANTrainOps:
    """What define_train_ops returns: the ordered phases (tfgan sequential hooks), LR schedules, and `run_step`,
    the counterpart of one `session.run(global_step_inc_op)` with its RunTrainOpsHook sequence
    (gan_train_for_shadow.py:141-142)."""

    def __init__(self, loss, lrs, ctx, use_pool=True):
        self.loss = loss
        self.lrs = lrs
        self.ctx = ctx
        if not ctx.group_affinity:  # the variable groups of one train op next to each other in the flat buffers
            ctx.group_affinity = [list(p.train_groups) for p in loss.phases]
        self.pools = {}
        self.use_pool = use_pool
        self.last_losses = {}
        self.capture_graphs = True
        self.pool_override = None  # tests: callable(name, fresh) -> tensor fed to the discriminator

    def _compiled(self, sess, phase, nb):
        ct = sess.compile_phase(self.loss.tower, nb, terms=phase.terms, train_groups=phase.train_groups,
                                key=phase.name)
        if self.capture_graphs and getattr(sess.backend, "name", "") == "hip" and ct._graph_all is None:
            ct.capture()
        return ct

    def _feed(self, ct, x, y, fed=None):
        """Copy the batch into the phase's input buffers.  The buffers are shared between the phases of a session
        (PhasePlan); `fed` (a set owned by one run_step call) makes only the first phase that reads an input pay for
        the copy."""
        b = ct.plan.buffers
        todo = []
        for name, t in (("x", x), ("y", y)):
            if "in:" + name in b:
                key = (name, b["in:" + name].data_ptr())
                if fed is None or key not in fed:
                    todo.append((name, t))
                    if fed is not None:
                        fed.add(key)
        ct.set_inputs(todo)  # (both batches in one launch)

    def run_step(self, x, y):
        sess = self.ctx.session()
        fed = set()
        nb = x.shape[0]
        step = sess.global_step
        for phase in self.loss.phases:
            ct = self._compiled(sess, phase, nb)
            self._feed(ct, x, y, fed)
            if phase.pool:
                gen = sess.compile_phase(self.loss.tower, nb, outputs=[t for _, t in phase.pool], key="generate")
                self._feed(gen, x, y, fed)
                gen.forward()
                pooled = []
                for name, t in phase.pool:
                    fresh = gen.value(t, copy=False)  # consumed (pool query / set_input copy) before the next forward
                    if self.pool_override is not None:
                        val = self.pool_override(name, fresh)
                    elif self.use_pool:
                        val = self.pools.setdefault(name, TensorPool(seed=sess.seed)).query(fresh)
                    else:
                        val = fresh
                    pooled.append((name, val))
                ct.set_inputs(pooled)
            ct.forward_backward()
            sess.allreduce_group_gradients(phase.train_groups)
            sess.adam_step_groups(phase.train_groups, self.lrs[phase.lr_key](step), step + 1, beta1=0.5)
            self.last_losses[phase.name] = ct
        sess.global_step += 1

    def losses(self):
        return {k: ct.loss_value() for k, ct in self.last_losses.items()}

    def close(self):
        """End of an episode: the pooled batches, the compiled phases and the device session (GanContext.close)."""
        self.pools.clear()
        self.last_losses.clear()
        self.ctx.close()


class GanContext:
    """Holds the recorded tower's variable store and (lazily) the device session."""

    def __init__(self, tower, backend=None, seed=1234):
        self.tower = tower
        self.backend = backend
        self.seed = seed
        self.group_affinity = []
        self._session = None

    def session(self):
        if self._session is None:
            from hypelcnn_amd.runtime import Session
            if self.backend is None:
                from hypelcnn_amd.backend import HipBackend
                self.backend = HipBackend()
            self._session = Session(self.tower.store, self.backend, seed=self.seed)
            self._session.finalize_variables(group_affinity=self.group_affinity)
            self._session.init_data_parallel()
        return self._session

    def close(self):
        """Release the device session (runtime.Session.close); session() would start a fresh one."""
        if self._session is not None:
            self._session.close()
            self._session = None


def define_standard_train_ops(gan_model, gan_loss, max_number_of_steps, generator_lr, discriminator_lr, backend=None):
    """reference :247-279: Adam(beta1=0.5) for generator and discriminator, sequential G-then-D phases."""
    lrs = {"gen": _get_lr(generator_lr, max_number_of_steps), "dis": _get_lr(discriminator_lr, max_number_of_steps)}
    return GANTrainOps(gan_loss, lrs, GanContext(gan_loss.tower, backend))


def ls_terms_generator(d_gen):
    return [G.LossTerm("mean_sq", d_gen, target=1.0, weight=0.5)]


def ls_terms_discriminator(d_real, d_gen):
    return [G.LossTerm("mean_sq", d_real, target=1.0, weight=0.5), G.LossTerm("mean_sq", d_gen, target=0.0, weight=0.5)]


# ----------------------------------------------------------------------------- checkpoint scoring (reference :47-219)
def restore_generators(ctx, restorer, variables):
    """create_generator_restorer().restore(sess, path): the checkpoint variables the wrapper's restorer selects, into
    the session of `ctx` (names the inference tower does not hold are skipped, as the reference's Saver only lists
    the graph's own variables)."""
    sess = ctx.session()
    for name in restorer(list(variables)):
        if name in sess.store.vars:
            sess.set_variable(name, variables[name])
    return sess


class BestRatioHolder:
    """The `max_size` best (lowest) divergences with their iterations, ascending; a new point goes in front of equal
    ones."""

    def __init__(self, max_size):
        self.data_holder = []
        self.max_size = max_size

    def add_point(self, iteration, diver_val):
        iteration = int(iteration)
        diver_val = float(diver_val)
        insert_idx = sum(1 for _, curr_diver in self.data_holder if diver_val > curr_diver)
        self.data_holder.insert(insert_idx, (iteration, diver_val))
        if len(self.data_holder) > self.max_size:
            self.data_holder.pop()

    def get_best_diver(self):
        return self.data_holder[0][1] if self.data_holder else None

    def get_point_with_itr(self, iteration):
        for curr_iter, curr_diver in self.data_holder:
            if curr_iter == iteration:
                return curr_iter, curr_diver
        return None, None

    def load(self, file_address):
        try:
            with open(file_address, "rb") as read_file:
                self.data_holder = json.load(read_file)
            print(f"Best ratio file {file_address} is loaded.", self.data_holder)
        except IOError:
            print(f"File {file_address} file not found. No best ratio is loaded.")
        except JSONDecodeError:
            print(f"File {file_address} file can not be decoded. No best ratio is loaded.")

    def save(self, file_address):
        with open(file_address, "w") as write_file:
            write_file.write(json.dumps(self.data_holder))

    @staticmethod
    def create_common_iterations(ratio_holder_1, ratio_holder_2):
        result = BestRatioHolder(ratio_holder_1.max_size)
        for curr_iter, _ in ratio_holder_1.data_holder:
            found_itr, found_kl = ratio_holder_2.get_point_with_itr(curr_iter)
            if found_itr is not None:
                result.add_point(found_itr, found_kl)
        return result

    def __str__(self):
        return str(self.data_holder)


class BaseValidationHook:
    def __init__(self, iteration_freq, log_dir, shadow_ratio):
        self._iteration_frequency = iteration_freq
        self._shadow_ratio = shadow_ratio
        self._log_dir = log_dir
        self.best_mean_div_holder = BestRatioHolder(10)
        self.best_upper_div_holder = BestRatioHolder(10)
        self.validation_itr_mark = False

    def after_create_session(self, session=None, coord=None):
        pass

    # the reference's hook fires on the iteration AFTER a multiple of the frequency (and so never on the last step of a
    # run); a hook installed on a training session here (--validate_while_training) fires on the multiples themselves:
    # the steps that are checkpointed, the closing step included, so that best_ratio_*.json names existing checkpoints
    on_checkpoint_steps = False

    def _is_validation_itr(self, current_iteration):
        if self._iteration_frequency != 0:
            if self.on_checkpoint_steps:
                return current_iteration % self._iteration_frequency == 0
            return current_iteration % self._iteration_frequency == 1 and current_iteration != 1
        return True

    def get_best_mean_div(self):
        return self.best_mean_div_holder.get_best_diver()

    def get_best_upper_div(self):
        return self.best_upper_div_holder.get_best_diver()


class PeerValidationHook:
    """The shadowed and de-shadowed hooks of a two-generator GAN, run together; prints the iterations both rank."""

    def __init__(self, *validation_base_hooks):
        self._validation_base_hooks = validation_base_hooks

    @property
    def band_ratio_stats(self):
        return all(hook.band_ratio_stats for hook in self._validation_base_hooks)

    @band_ratio_stats.setter
    def band_ratio_stats(self, on):
        for hook in self._validation_base_hooks:
            hook.band_ratio_stats = on

    def on_training_session(self, write_files=True):
        for hook in self._validation_base_hooks:
            hook.on_training_session(write_files)
        return self

    def after_create_session(self, session=None, coord=None):
        for hook in self._validation_base_hooks:
            hook.after_create_session(session, coord)

    def after_run(self, current_iteration=0):
        ratio_holder_list = []
        for hook in self._validation_base_hooks:
            hook.after_run(current_iteration)
            ratio_holder_list.append(hook.best_mean_div_holder)
        if self._validation_base_hooks[0].validation_itr_mark:
            print("Best common options:",
                  BestRatioHolder.create_common_iterations(ratio_holder_list[0], ratio_holder_list[1]))

    def get_best_mean_div(self):
        return [h.get_best_mean_div() for h in self._validation_base_hooks if h.get_best_mean_div() is not None]

    def get_best_upper_div(self):
        return [h.get_best_upper_div() for h in self._validation_base_hooks if h.get_best_upper_div() is not None]

    def last_divergences(self):
        return [d for h in self._validation_base_hooks for d in h.last_divergences()]


class ValidationHook(BaseValidationHook):
    """Runs the generator `infer_model` (a symbol of the tower of `ctx`, fed through the placeholder `input_tensor`) on
    `sample_count` fixed pixels of one side of the shadow map and tracks create_stats' divergences;
    best_ratio_<suffix>.json and a line of log_dir/summaries.jsonl record the result.  With `band_ratio_stats` set
    (--band_ratio_stats true; off by default, when no file is added), every validation iteration also writes the
    reference's band-ratio figure (print_stats :210-219) as band_ratio_<suffix>_<iteration>.pdf -- the per-band median
    of generated / input * ratio with the 10th to 90th percentile band -- and its numbers as
    band_ratio_<suffix>_<iteration>.json (common/band_ratio.py: the percentiles are selected on the device from the
    generated tensor where it is)."""

    band_ratio_stats = False
    write_files = True  # data parallel: every rank validates (the same parameters), only the chief writes

    def __init__(self, iteration_freq, sample_count, log_dir, loader, data_set, neighborhood, shadow_map, shadow_ratio,
                 input_tensor, infer_model, name_suffix, fetch_shadows, ctx, seed=1234, device_samples=False):
        """device_samples: take the samples of a device-resident scene (common/device_scene.py) where they are -- one
        gather on the device -- instead of through get_data_point, which downloads the scene."""
        super().__init__(iteration_freq, log_dir, shadow_ratio)
        self._ctx = ctx
        self._infer_model = infer_model
        self._input_tensor = input_tensor
        self._name_suffix = name_suffix
        self._best_mean_div_addr = os.path.join(self._log_dir, f"best_ratio_{name_suffix}.json")
        self.best_mean_div_holder.load(self._best_mean_div_addr)
        self._bands = loader.get_band_measurements()
        self.sample_indices = sample_indices_for_testing(sample_count, neighborhood, shadow_map, fetch_shadows,
                                                         numpy.random.default_rng(seed))
        self._data_sample_list = load_samples_on_device(data_set, self.sample_indices) if device_samples else \
            load_samples_for_testing(data_set, self.sample_indices)
        self.last_stats = None

    def on_training_session(self, write_files=True):
        """The hook rides on a training session (--validate_while_training): it fires on the checkpointed steps, and
        only the chief rank writes."""
        self.on_checkpoint_steps = True
        self.write_files = bool(write_files)
        return self

    def last_divergences(self):
        """[mean divergence] of the last validation run ([] before one)"""
        return [] if self.last_stats is None else [self.last_stats[0]]

    def after_run(self, current_iteration=0):
        self.validation_itr_mark = self._is_validation_itr(current_iteration)
        if not self.validation_itr_mark:
            return
        from hypelcnn_amd.gan.gan_train_for_shadow import create_stats
        sess = self._ctx.session()
        n = self._data_sample_list.shape[0]
        ct = sess.compile_phase(self._ctx.tower, n, outputs=[self._infer_model], key="validate_" + self._name_suffix)
        x = torch.as_tensor(self._data_sample_list).to(sess.backend.device)
        ct.set_input(self._input_tensor.name, x)
        ct.forward()
        generated = ct.value(self._infer_model, copy=False)
        ratio = torch.as_tensor(numpy.asarray(self._shadow_ratio, numpy.float32)).to(x.device)
        div_mean, div_upper, mean, std = create_stats(generated, x, ratio)
        self.last_stats = (div_mean, div_upper, mean.cpu().numpy(), std.cpu().numpy())
        self.best_mean_div_holder.add_point(current_iteration, div_mean)
        self.best_upper_div_holder.add_point(current_iteration, div_upper)
        if self.write_files:
            self.best_mean_div_holder.save(self._best_mean_div_addr)
            with open(os.path.join(self._log_dir, "summaries.jsonl"), "a") as f:
                f.write(json.dumps({"step": int(current_iteration), f"divergence_{self._name_suffix}": div_mean}) + "\n")
        print(f"Validation metrics for {self._name_suffix} #{current_iteration}")
        print_overall_info(self.last_stats[2], self.last_stats[3])
        if self.band_ratio_stats and self.write_files:
            from hypelcnn_amd.common.band_ratio import band_ratio_stats, write_band_ratio
            self.last_band_ratio = write_band_ratio(
                self._log_dir, f"band_ratio_{self._name_suffix}", current_iteration, self._bands,
                band_ratio_stats(sess.backend, generated, x, ratio), "p50", "p10", "p90")
        print(f"Divergence for {self._name_suffix}; mean:{div_mean}, upper:{div_upper}")
        print(f"Best {self._name_suffix} options:{self.best_mean_div_holder}")


def create_one_way_training_hook(model, train_ops, fetch_shadows, images_x, images_y, data_set, loader, log_dir,
                                 neighborhood, shadow_map, shadow_ratio, validation_iteration_count,
                                 validation_sample_count, device_samples=False):
    """The hook of a one-generator model (gan_x2y / gan_y2x, cut_x2y / cut_y2x) on the TRAINING tower's own symbols and
    session: the model's generated_data from the placeholder it is fed by -- y and the shadowed pixels with the inverse
    ratio when the inputs are swapped (what GANInferenceWrapper.create_inference_hook builds on a tower of its own)."""
    return ValidationHook(iteration_freq=validation_iteration_count, sample_count=validation_sample_count,
                          log_dir=log_dir, loader=loader, data_set=data_set, neighborhood=neighborhood,
                          shadow_map=shadow_map, shadow_ratio=adj_shadow_ratio(shadow_ratio, fetch_shadows),
                          input_tensor=images_y if fetch_shadows else images_x, infer_model=model.generated_data,
                          fetch_shadows=fetch_shadows, name_suffix="deshadowed" if fetch_shadows else "shadowed",
                          ctx=train_ops.ctx, device_samples=device_samples)


def sample_indices_for_testing(sample_count, neighborhood, shadow_map, fetch_shadows, rng):
    """The (x, y) scene coordinates load_samples_for_testing (reference :362-382) draws, with replacement, from the
    shadowed (> 0) or lit (== 0) pixels of the unpadded map.  Drawn with a seeded NumPy generator instead of Python's
    `random`, so the sample is reproducible; the distribution is the same."""
    if neighborhood > 0:
        shadow_map = shadow_map[neighborhood:-neighborhood, neighborhood:-neighborhood]
    indices = numpy.where(shadow_map > 0) if fetch_shadows else numpy.where(shadow_map == 0)
    picks = rng.integers(0, indices[0].size, size=sample_count)
    return numpy.stack([indices[1][picks], indices[0][picks]], axis=1)


def load_samples_for_testing(data_set, sample_indices):
    """[n, bands] float32: the spectrum of each (x, y) (neighbourhood 0: the reference's squeeze(axis=[1, 2]))."""
    band_size = data_set.get_casi_band_count()
    samples = [data_set.get_data_point(int(x), int(y))[:, :, 0:band_size] for x, y in sample_indices]
    return numpy.ascontiguousarray(numpy.asarray(samples, numpy.float32).reshape(len(samples), band_size))


def load_samples_on_device(data_set, sample_indices):
    """load_samples_for_testing for a device-resident scene at neighbourhood 0: [n, bands] float32 gathered from the
    prepared raster where it is (a device tensor; the scene is not downloaded)."""
    n = int(data_set.neighborhood)
    if n != 0:
        raise ValueError("load_samples_on_device takes single spectra: a scene prepared with neighborhood 0")
    casi = data_set.casi_dev
    idx = torch.as_tensor(numpy.ascontiguousarray(sample_indices), dtype=torch.long).to(casi.device)
    return casi[idx[:, 1], idx[:, 0], :data_set.get_casi_band_count()].contiguous()


def print_overall_info(mean, std):
    print("Mean&std Generated vs Original Ratio: ")
    band_size = mean.shape[0]
    for band_index in range(0, band_size):
        prefix = "[ " if band_index == 0 else ""
        postfix = " ]" if band_index == band_size - 1 and band_index != 0 else ""
        print(f"{prefix}{mean[band_index]:2.4f}\u00B1{std[band_index]:2.2f}{postfix}",
              end="\n" if band_index % 5 == 1 else " ")
