"""Training on the HIP engine: model_fn's TRAIN / EVAL branches (code/utils/generate_model.py:697-830,
"GM") and the loop of train_and_evaluate (code/utils/framework_operations.py:108-166, "FO").

* loss: ``learning_options.loss`` (GM:745-753) over the batch's concatenated flat predictions,
  plus the Dense l2 kernel regularizers (AUX:833-834).  The engine computes it through ``ign_loss``:
  MeanSquaredError (kind 0, which ``ign_mse_loss`` names), MeanAbsoluteError,
  MeanAbsolutePercentageError, MeanSquaredLogarithmicError, Huber, LogCosh, BinaryCrossentropy and
  Poisson with Keras' default constructor arguments; ``ign_l2_loss`` for the regularizers.
* gradients: ``ign_backward``, the HIP backward of the whole forward (tf.gradients, GM:790).
* optimizer: ``learning_options.optimizer`` (GM:797-818), Keras optimizer_v2 semantics, through
  ``ign_optimizer_step``: Adam (kind 0, which ``ign_adam_step`` names), SGD (momentum, nesterov),
  RMSprop (momentum, centered), Adagrad, Adadelta and Adamax.  Nadam, Ftrl, amsgrad and gradient clipping
  are refused.  The learning rate is a float (default: the optimizer's own) or an ExponentialDecay,
  PiecewiseConstantDecay, PolynomialDecay or InverseTimeDecay schedule evaluated at ``iterations``
  (the global step, GM:816).
* ``learning_options(model_info)`` parses all of this without a GPU and raises UnsupportedModel
  for what is not lowered.
* data parallel: with torch.distributed initialised, every rank trains on its own batches and
  the gradient is averaged with one all-reduce (RCCL on GPUs) before the update.
* resuming: ``Trainer.state()`` / ``load_state()`` carry the parameters, the optimizer's slots by
  parameter name, ``iterations`` and the dropout seed, so a new Trainer continues a run bit for bit
  (the Estimator restores the same from model_dir); ``check_finite`` counts NaN / Inf gradient values
  on the GPU (``ign_nonfinite_count``) and raises NonFiniteTraining (the Estimator's NanTensorHook).
* eval metrics (GM:755-785): label/prediction mean, MAE, MRE and the batch-mean r-squared
  (GM:201-216), after denormalisation, plus the mean loss.
"""

from __future__ import annotations

import ctypes as C
import math
import os
import time

import numpy as np

from .engine import UnsupportedModel
from .generate_model import ComnetModel, _resolve

SUPPORTED_LOSSES = ("MeanSquaredError", "MeanAbsoluteError", "MeanAbsolutePercentageError",
                    "MeanSquaredLogarithmicError", "Huber", "LogCosh", "BinaryCrossentropy", "Poisson")
SUPPORTED_SCHEDULES = ("ExponentialDecay", "PiecewiseConstantDecay", "PolynomialDecay", "InverseTimeDecay")

# per optimizer: the hyper-parameters its Keras constructor takes beside learning_rate / name, with
# Keras' defaults, and the default constant rate
_OPTIMIZERS = {
    "Adam": ({"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7}, 0.001),
    "SGD": ({"momentum": 0.0, "nesterov": False}, 0.01),
    "RMSprop": ({"rho": 0.9, "momentum": 0.0, "epsilon": 1e-7, "centered": False}, 0.001),
    "Adagrad": ({"initial_accumulator_value": 0.1, "epsilon": 1e-7}, 0.001),
    "Adadelta": ({"rho": 0.95, "epsilon": 1e-7}, 0.001),
    "Adamax": ({"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7}, 0.001),
}
_REFUSED_KEYS = ("clipnorm", "clipvalue", "global_clipnorm")


class LearningRate:
    """``optimizer.learning_rate`` or ``optimizer.schedule`` (Keras ExponentialDecay,
    PiecewiseConstantDecay, PolynomialDecay, InverseTimeDecay), evaluated on the host at the step.
    ``default``: the optimizer's own Keras rate where ``learning_rate`` is absent."""

    def __init__(self, opt: dict, default: float = 0.001):
        sched = opt.get("schedule")
        self.kind = "constant"
        self.lr0 = float(opt.get("learning_rate", default))
        if sched is not None:
            sched = dict(sched)
            kind = sched.pop("type")
            if kind not in SUPPORTED_SCHEDULES:
                raise UnsupportedModel("learning-rate schedule %r is not lowered (%s)" % (kind, ", ".join(SUPPORTED_SCHEDULES)))
            self.kind = kind
            if kind == "PiecewiseConstantDecay":
                self.boundaries = [float(b) for b in sched["boundaries"]]
                self.values = [float(v) for v in sched["values"]]
                if len(self.values) != len(self.boundaries) + 1:   # Keras' own check
                    raise ValueError("PiecewiseConstantDecay: %d values for %d boundaries (one more is needed)"
                                     % (len(self.values), len(self.boundaries)))
                self.lr0 = self.values[0]
                return
            self.lr0 = float(sched["initial_learning_rate"])
            self.decay_steps = float(sched["decay_steps"])
            if kind == "PolynomialDecay":
                self.end = float(sched.get("end_learning_rate", 1e-4))
                self.power = float(sched.get("power", 1.0))
                self.cycle = bool(sched.get("cycle", False))
                return
            self.decay_rate = float(sched["decay_rate"])
            # Keras tests `if self.staircase:`; a JSON string such as "True" (QSJ:204) or even
            # "False" is truthy there
            self.staircase = bool(sched.get("staircase", False))

    def __call__(self, step: int) -> float:
        if self.kind == "constant":
            return self.lr0
        if self.kind == "PiecewiseConstantDecay":
            for b, v in zip(self.boundaries, self.values):
                if step <= b:
                    return v
            return self.values[-1]
        if self.kind == "PolynomialDecay":
            steps = self.decay_steps
            if self.cycle:
                steps *= max(1, math.ceil(step / self.decay_steps))
            else:
                step = min(step, steps)
            return (self.lr0 - self.end) * (1 - step / steps) ** self.power + self.end
        p = step / self.decay_steps
        if self.staircase:
            p = math.floor(p)
        if self.kind == "InverseTimeDecay":
            return self.lr0 / (1 + self.decay_rate * p)
        return self.lr0 * self.decay_rate ** p


class LearningOptions:
    """``learning_options`` lowered: ``loss`` / ``loss_kind`` (ign_loss_kind), ``optimizer`` /
    ``desc`` (an ``_lib.OptimizerDesc``), its ``num_slots`` buffers starting at ``slot_init``, the
    hyper-parameters as given or defaulted (``hyper``) and the ``lr`` schedule."""

    def __init__(self, loss, loss_kind, optimizer, desc, num_slots, slot_init, hyper, lr):
        self.loss, self.loss_kind, self.optimizer, self.desc = loss, loss_kind, optimizer, desc
        self.num_slots, self.slot_init, self.hyper, self.lr = num_slots, slot_init, hyper, lr


def _kind(fn, name) -> int:
    from . import _lib
    k = _lib.i32()
    rc = fn(str(name).encode(), C.byref(k))
    if rc != 0:   # the library's message lists the supported names
        raise UnsupportedModel(_lib.lib.ign_last_error().decode(errors="replace"))
    return k.value


def learning_options(model_info) -> LearningOptions:
    """``learning_options`` of a model description -> LearningOptions, without a GPU.  Raises
    UnsupportedModel for a loss, optimizer or schedule that is not lowered, for gradient clipping
    and Adam's amsgrad, and for a key the (non-Adam) optimizer's Keras constructor does not take."""
    from . import _lib
    loss = model_info.get_loss()
    loss_kind = _kind(_lib.lib.ign_loss_kind, loss)
    opt = dict(model_info.get_optimizer())
    name = opt.get("type")
    kind = _kind(_lib.lib.ign_optimizer_kind, name)
    defaults, rate = _OPTIMIZERS[name]
    for k in _REFUSED_KEYS:
        if k in opt:
            raise UnsupportedModel("optimizer option %r is not lowered (gradient clipping)" % k)
    if name == "Adam":
        if opt.get("amsgrad"):
            raise UnsupportedModel("Adam's amsgrad is not lowered")
    else:
        unknown = sorted(set(opt) - set(defaults) - {"type", "schedule", "learning_rate", "name"})
        if unknown:
            raise UnsupportedModel("%s does not take %s (its Keras constructor: learning_rate, %s)"
                                   % (name, ", ".join(repr(k) for k in unknown), ", ".join(defaults)))
    hyper = {k: type(d)(opt.get(k, d)) if not isinstance(d, bool) else bool(opt.get(k, d)) for k, d in defaults.items()}
    desc = _lib.OptimizerDesc(kind=kind, nesterov=int(hyper.get("nesterov", False)), centered=int(hyper.get("centered", False)),
                              reserved=0, momentum=hyper.get("momentum", 0.0), rho=hyper.get("rho", 0.0),
                              beta_1=hyper.get("beta_1", 0.0), beta_2=hyper.get("beta_2", 0.0),
                              epsilon=hyper.get("epsilon", 0.0),
                              initial_accumulator_value=hyper.get("initial_accumulator_value", 0.0))
    if hyper.get("momentum", 0.0) < 0 or hyper.get("momentum", 0.0) > 1:   # Keras' own check
        raise ValueError("momentum must be between 0 and 1")
    n, init = _lib.i32(), _lib.f32()
    _lib.check(_lib.lib.ign_optimizer_num_slots(C.byref(desc), C.byref(n), C.byref(init)))
    return LearningOptions(loss, loss_kind, name, desc, n.value, init.value, hyper, LearningRate(opt, rate))


def host_loss(kind: int, p, y) -> float:
    """The loss of ``kind`` in float64 on the host (Keras' default constructor arguments), as the
    engine's ign_loss defines it: the mean over the flat predictions."""
    p, y = np.asarray(p, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    eps, d = 1e-7, p - y
    name = SUPPORTED_LOSSES[kind]
    if name == "MeanSquaredError":
        t = d * d
    elif name == "MeanAbsoluteError":
        t = np.abs(d)
    elif name == "MeanAbsolutePercentageError":
        t = 100.0 * np.abs(d) / np.maximum(np.abs(y), eps)
    elif name == "MeanSquaredLogarithmicError":
        t = (np.log1p(np.maximum(p, eps)) - np.log1p(np.maximum(y, eps))) ** 2
    elif name == "Huber":
        t = np.where(np.abs(d) <= 1.0, 0.5 * d * d, np.abs(d) - 0.5)
    elif name == "LogCosh":
        t = np.abs(d) + np.log1p(np.exp(-2.0 * np.abs(d))) - math.log(2.0)
    elif name == "BinaryCrossentropy":
        q = np.clip(p, eps, 1.0 - eps)
        t = -(y * np.log(q + eps) + (1.0 - y) * np.log(1.0 - q + eps))
    else:
        t = p - y * np.log(p + eps)
    return float(np.mean(t))


class NonFiniteTraining(FloatingPointError):
    """A NaN or Inf reached the gradient, the loss, the parameters or an optimizer slot (the
    Estimator's NanTensorHook).  The device counter is read only where the host waits anyway, so the
    first bad step lies in ``first_possible_step .. detected_step``: the step after the last clean
    reading, and the step the host had reached when it read the counter."""

    def __init__(self, what: str, first_possible_step: int, detected_step: int):
        super().__init__("training went non-finite: %s (first possible step %d, detected at step %d)"
                         % (what, first_possible_step, detected_step))
        self.first_possible_step, self.detected_step = int(first_possible_step), int(detected_step)


STATE_FORMAT = 1
_GOLDEN = 0x9E3779B97F4A7C15


def slot_names(optimizer: str, hyper: dict) -> list:
    """Keras' slot names of ``optimizer``'s buffers, in ign_optimizer_num_slots' order."""
    if optimizer in ("Adam", "Adamax"):
        return ["m", "v"]
    if optimizer == "SGD":
        return ["momentum"] if hyper.get("momentum", 0.0) > 0 else []
    if optimizer == "RMSprop":   # the engine's order: rms, then mg (centered), then momentum
        return ["rms"] + (["mg"] if hyper.get("centered") else []) + (["momentum"] if hyper.get("momentum", 0.0) > 0 else [])
    if optimizer == "Adagrad":
        return ["accumulator"]
    if optimizer == "Adadelta":
        return ["accum_grad", "accum_var"]
    raise UnsupportedModel("optimizer %r is not lowered" % (optimizer,))


def cut_flat(flat, layout, suffix: str = "") -> dict:
    """A flat buffer in the plan's parameter layout ([(name, shape, offset)], ``Engine.layout``) ->
    {name + suffix: tensor}; the alignment gaps between the tensors are dropped."""
    flat = np.asarray(flat)
    return {name + suffix: flat[off:off + int(np.prod(shape))].reshape(shape).copy() for name, shape, off in layout}


def fill_flat(tensors: dict, layout, n: int, fill: float = 0.0, suffix: str = "") -> np.ndarray:
    """The inverse of ``cut_flat``: a flat float32 buffer of ``n`` values, the gaps holding ``fill``."""
    flat = np.full(n, fill, np.float32)
    for name, shape, off in layout:
        flat[off:off + int(np.prod(shape))] = np.asarray(tensors[name + suffix], np.float32).reshape(-1)
    return flat


def state_meta(options: LearningOptions, iterations: int, dropout_seed: int) -> dict:
    """The metadata of a training state: what ``unpack_state`` holds a loading run to."""
    return {"format": STATE_FORMAT, "iterations": int(iterations), "dropout_seed": int(dropout_seed),
            "optimizer": options.optimizer, "hyper": dict(options.hyper), "slot_init": float(options.slot_init),
            "loss": options.loss}


def pack_state(params: dict, slots: list, options: LearningOptions, layout, iterations: int, dropout_seed: int) -> dict:
    """{"tensors", "meta"} from the named parameters and the optimizer's flat slot buffers (host arrays
    in ``layout``): each slot is cut into ``<param name>/<Optimizer>/<slot>`` tensors."""
    tensors = {name: np.asarray(params[name], np.float32) for name, _, _ in layout}
    for slot, flat in zip(slot_names(options.optimizer, options.hyper), slots):
        tensors.update(cut_flat(flat, layout, "/%s/%s" % (options.optimizer, slot)))
    return {"tensors": tensors, "meta": state_meta(options, iterations, dropout_seed)}


def unpack_state(state: dict, options: LearningOptions, layout, n: int):
    """(parameters, flat slot buffers) of a training state for a run with ``options`` and the plan
    ``layout`` of ``n`` values (gaps hold the optimizer's slot_init).  ValueError when the state is
    another optimizer's or differs in a hyper-parameter, lacks a tensor or has one too many, or holds a
    tensor of another shape (what the reference's Saver.restore refuses too)."""
    meta, tensors = state["meta"], state["tensors"]
    if meta.get("format") != STATE_FORMAT:
        raise ValueError("load_state: state format %r, this version reads format %d" % (meta.get("format"), STATE_FORMAT))
    if meta["optimizer"] != options.optimizer:
        raise ValueError("load_state: the state was trained with optimizer %s, the model description names %s"
                         % (meta["optimizer"], options.optimizer))
    if meta["loss"] != options.loss:
        raise ValueError("load_state: the state was trained with loss %s, the model description names %s"
                         % (meta["loss"], options.loss))
    for k in sorted(set(meta["hyper"]) | set(options.hyper)):
        if k not in meta["hyper"] or k not in options.hyper or meta["hyper"][k] != options.hyper[k]:
            raise ValueError("load_state: hyper-parameter %s is %r in the state and %r in the model description"
                             % (k, meta["hyper"].get(k), options.hyper.get(k)))
    suffixes = [""] + ["/%s/%s" % (options.optimizer, s) for s in slot_names(options.optimizer, options.hyper)]
    want = {name + sfx: tuple(shape) for sfx in suffixes for name, shape, _ in layout}
    missing = sorted(set(want) - set(tensors))
    if missing:
        raise ValueError("load_state: the state lacks tensor(s) %s" % ", ".join(missing))
    extra = sorted(set(tensors) - set(want))
    if extra:
        raise ValueError("load_state: the state holds tensor(s) the model does not have: %s" % ", ".join(extra))
    for name, shape in want.items():
        if tuple(np.shape(tensors[name])) != shape:
            raise ValueError("load_state: %s has shape %s in the state, the model needs %s"
                             % (name, tuple(np.shape(tensors[name])), shape))
    params = {name: np.asarray(tensors[name], np.float32) for name, _, _ in layout}
    slots = [fill_flat(tensors, layout, n, meta["slot_init"], sfx) for sfx in suffixes[1:]]
    return params, slots


class Trainer:
    def __init__(self, model_info, params: dict | None = None, device: int = 0, seed: int = 0, dist=None,
                 check_finite: bool = False):
        lo = learning_options(model_info)   # refuses what is not lowered before torch or the GPU are touched
        import torch
        self.torch = torch
        self.options = lo
        self.loss_kind = lo.loss_kind
        self.lr = lo.lr
        self.model_info = model_info
        torch.cuda.set_device(device)
        self.model = ComnetModel(model_info, device=device, params=params, seed=seed)
        eng = self.model.engine
        eng.set_stream(torch.cuda.current_stream().cuda_stream)   # torch copies / RCCL stream-ordered
        dev = torch.device("cuda", device)
        self.grads = torch.zeros(eng.n_params, dtype=torch.float32, device=dev)
        # the optimizer's slot buffers (ign_optimizer_num_slots' order, all starting at its value:
        # Adagrad's accumulator, alignment gaps included); Adam's moments are also m and v
        self.slots = [torch.full_like(self.grads, lo.slot_init) for _ in range(lo.num_slots)]
        self.m, self.v = self.slots if lo.optimizer == "Adam" else (None, None)
        self.dpred = None
        self.device = dev
        self.dist = dist
        self.iterations = 0
        # the Dropout mask stream: the trainer's seed mixed with the data-parallel rank (ranks draw
        # different masks); the step number is ``iterations``, so a run resumed at step k (load_state
        # restores both) redraws step k's
        self._rank = dist.get_rank() if dist is not None and dist.is_initialized() else 0
        self._set_dropout_seed(seed)
        # check_finite: every step adds its gradient's NaN / Inf count to one device counter
        # (ign_nonfinite_count, enqueued, no wait); the host reads it where it waits anyway
        self.check_finite = bool(check_finite)
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=dev) if self.check_finite else None
        self._clean_through = 0   # the counter read zero with this many steps enqueued
        # IGN_STEP_PROF=1: host seconds per phase of train_prepared (bench.py --fresh-batches reports them)
        self.step_prof = (dict.fromkeys(("forward_enqueue", "loss_wait", "backward_enqueue", "close", "l2_wait",
                                         "steps"), 0.0) if os.environ.get("IGN_STEP_PROF") == "1" else None)
        self.output_name, _, self.output_denorm = model_info.get_output_info()

    @property
    def engine(self):
        return self.model.engine

    def _set_dropout_seed(self, base: int):
        """``base``: the seed every rank was given (what a state file stores); the rank is mixed in."""
        self.base_dropout_seed = int(base) & 0xFFFFFFFFFFFFFFFF
        self.dropout_seed = (int(base) + _GOLDEN * self._rank) & 0xFFFFFFFFFFFFFFFF

    def _check_counter(self, detected_step: int):
        """Read the gradient counter (a host wait: call it where the stream is waited for anyway)."""
        if not self.check_finite:
            return
        bad = int(self.nonfinite.item()) & 0xFFFFFFFF
        if bad:
            raise NonFiniteTraining("%d NaN / Inf gradient value(s)" % bad, self._clean_through + 1, detected_step)
        self._clean_through = self.iterations

    def check_now(self):
        """Wait for the enqueued steps and raise NonFiniteTraining if one of their gradients held a NaN
        or Inf (nothing without ``check_finite``): for the ranks that do not call ``state()``."""
        self._check_counter(self.iterations)

    def _labels(self, labels):
        y = np.concatenate([np.asarray(l, np.float32).reshape(-1) for l in labels])
        return self.torch.from_numpy(y).to(self.device)

    def prepare(self, features, labels):
        """The host half of a step: the batch (CSR tables, H2D copies, the training tables) and the
        device label vector.  Safe on a worker thread while the GPU runs another step (the engine
        builds batches on a non-blocking stream of the calling thread; the labels use a torch
        stream of their own)."""
        b = self.model.batch(features)
        try:
            b.enable_training()
            y = np.concatenate([np.asarray(l, np.float32).reshape(-1) for l in labels])
            if y.size != b.predictions * b.output_units:
                raise ValueError("labels hold %d values for %d predictions" % (y.size, b.predictions * b.output_units))
            torch = self.torch
            with torch.cuda.device(self.device):
                s = torch.cuda.Stream(self.device)
                with torch.cuda.stream(s):
                    yd = torch.from_numpy(y).pin_memory().to(self.device, non_blocking=True)
                s.synchronize()
        except BaseException:
            b.close()
            raise
        return b, yd

    def train_step(self, features: list, labels: list) -> dict:
        """One optimizer step on a batch of graphs (model_fn TRAIN, GM:712-830)."""
        return self.train_prepared(*self.prepare(features, labels))

    def train_prepared(self, b, y, want_loss: bool = True) -> dict:
        """One optimizer step on a batch made by ``prepare`` (closed here).  ``want_loss=False``: the
        step is only enqueued -- no host wait for the loss or the regularisation term (the returned
        dict has None for them), so the next step's host work overlaps this one on the GPU; the
        training loop asks for them on the steps it logs (tf.estimator computes the loss every step
        but only the logged steps reach the host)."""
        prof = self.step_prof
        tick = time.perf_counter if prof is not None else None
        t0 = tick() if tick else 0.0
        # y was made on a builder's stream: without a host wait in this step, its memory must not
        # return to that stream's pool before the step has read it
        y.record_stream(self.torch.cuda.current_stream(y.device))
        try:
            b.set_dropout(self.dropout_seed, self.iterations)
            b.forward_train(to_host=False)
            if tick:
                t1 = tick()
                prof["forward_enqueue"] += t1 - t0
            dpred = self.torch.empty_like(y)
            loss = self.engine.loss(self.loss_kind, b.predictions_ptr(), y, dpred, want_loss=want_loss)
            if tick:
                t2 = tick()
                prof["loss_wait"] += t2 - t1
            if self.check_finite and want_loss:
                # the stream was just waited for: the counter holds every earlier step's gradient
                self._check_counter(self.iterations + 1)
                if not math.isfinite(loss):
                    raise NonFiniteTraining("the loss is %r" % loss, self.iterations + 1, self.iterations + 1)
            # sum(model.losses) is part of this step's total loss (GM:749-753): read at the parameters the
            # step starts from, before the update below (the stream is idle here, the loss was just read)
            reg = self.engine.l2_loss() if want_loss else None
            if tick:
                t1 = tick()
                prof["l2_wait"] += t1 - t2
                t2 = t1
            b.backward(dpred, self.grads)
            if tick:
                t3 = tick()
                prof["backward_enqueue"] += t3 - t2
            if self.dist is not None and self.dist.is_initialized() and self.dist.get_world_size() > 1:
                if self.dist.get_backend() == "gloo":   # CPU collectives (tests, rehearsals): host-staged
                    g = self.grads.cpu()
                    self.dist.all_reduce(g)
                    self.grads.copy_(g)
                else:                                   # RCCL over xGMI
                    self.dist.all_reduce(self.grads)
                self.grads /= self.dist.get_world_size()
            if self.check_finite:
                self.engine.nonfinite_count(self.grads, self.nonfinite)
            lr = self.lr(self.iterations)
            self.engine.optimizer_step(self.options.desc, self.grads, self.slots, self.iterations, lr)
            self.iterations += 1
        finally:
            if tick:
                t4 = tick()
            b.close()
            if tick:
                t5 = tick()
                prof["close"] += t5 - t4
        if tick:
            prof["steps"] += 1
        return {"loss": loss, "regularization_loss": reg, "total_loss": loss + reg if want_loss else None,
                "learning_rate": lr, "step": self.iterations}

    def _denorm(self, v):
        if self.output_denorm is None or str(self.output_denorm) == "None":
            return v
        try:
            return _resolve(self.output_denorm)(v, self.output_name)
        except KeyError:
            return v

    def evaluate(self, batches) -> dict:
        """model_fn EVAL (GM:755-785) over an iterable of (features, labels) batches."""
        labels_all, preds_all, losses, r2 = [], [], [], []
        for features, labels in batches:
            b = self.model.batch(features)
            try:
                p = b.forward().reshape(-1).astype(np.float64)
            finally:
                b.close()
            y = np.concatenate([np.asarray(l, np.float64).reshape(-1) for l in labels])
            losses.append(host_loss(self.loss_kind, p, y))   # (kind 0: bitwise np.mean((y - p) ** 2))
            yd = np.asarray(self._denorm(y), np.float64)
            pd = np.asarray(self._denorm(p), np.float64)
            labels_all.append(yd)
            preds_all.append(pd)
            tot = np.sum((yd - yd.mean()) ** 2)
            r2.append(1.0 - np.sum((yd - pd) ** 2) / tot if tot > 0 else float("nan"))
        y = np.concatenate(labels_all)
        p = np.concatenate(preds_all)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(y != 0, np.abs(y - p) / np.abs(y), 0.0)   # div_no_nan
        return {"loss": float(np.mean(losses)), "label/mean": float(y.mean()), "prediction/mean": float(p.mean()),
                "mae": float(np.mean(np.abs(y - p))), "mre": float(rel.mean()), "r-squared": float(np.nanmean(r2)),
                "samples": int(len(losses))}

    def params(self) -> dict:
        return self.engine.get_params()

    def prefetch(self, jobs, depth: int = 2, workers: int = 1, load=None) -> "BatchPrefetcher":
        return BatchPrefetcher(self, jobs, depth, workers, load)

    def set_params(self, params: dict):
        self.model.set_params(params)

    def state(self) -> dict:
        """Everything a new Trainer of the same description needs to continue this run bit for bit
        (``load_state``): {"tensors": the parameters as ``params()`` gives them and every optimizer slot
        cut by the plan's parameter layout into ``<param name>/<Optimizer>/<slot>`` tensors (no
        alignment gaps), "meta": ``iterations``, the dropout seed before the rank is mixed in, the
        optimizer with its hyper-parameters and slot_init, the loss}.  Waits for the enqueued steps; with
        ``check_finite`` it raises NonFiniteTraining rather than return a state whose run saw a NaN or Inf
        gradient or whose host copies hold one."""
        params = self.params()                          # waits for the stream
        slots = [s.cpu().numpy() for s in self.slots]
        self._check_counter(self.iterations)
        st = pack_state(params, slots, self.options, self.engine.layout, self.iterations, self.base_dropout_seed)
        bad = [k for k, v in st["tensors"].items() if not np.isfinite(v).all()] if self.check_finite else []
        if bad:
            raise NonFiniteTraining("NaN / Inf in %s" % ", ".join(bad[:4]) + (" ..." if len(bad) > 4 else ""),
                                    self._clean_through + 1, self.iterations)
        return st

    def load_state(self, state: dict):
        """Continue the run ``state`` was taken from: the parameters, every slot tensor written back at
        its offset of this plan's layout (gaps get slot_init), ``iterations`` and the dropout seed.
        ValueError (``unpack_state``) for a state of another optimizer, hyper-parameter, tensor set or
        shape; nothing is changed then."""
        params, slots = unpack_state(state, self.options, self.engine.layout, self.engine.n_params)
        self.set_params(params)
        for dst, flat in zip(self.slots, slots):   # in place: m and v stay the Adam slots
            dst.copy_(self.torch.from_numpy(flat))
        self.iterations = int(state["meta"]["iterations"])
        self._set_dropout_seed(state["meta"]["dropout_seed"])
        if self.check_finite:
            self.nonfinite.zero_()
        self._clean_through = self.iterations


def builder_cpus(workers: int) -> list:
    """CPU sets for ``workers`` batch-builder threads (IGN_PIN_BUILDERS=1; default off): two CPUs each,
    consecutive ones of the NUMA node the calling thread runs on, within the process's affinity
    (local rank r of a multi-rank node takes the r-th slice).
    A builder's index tables are memory-bound host work; a thread the scheduler moved across CCDs
    and NUMA nodes between batches ran the ordered MP's message lists at 20-21 ms instead of
    10 ms pinned (one builder, `r06_c22.sh`).  With eight builders on a shared host it measured
    slower (24.0-26.6 against 19.0-23.9 ms per fresh-batch step, `r06_c23.sh`: the low CPUs it
    picks are other tenants' too), hence off by default.  Empty sets (no pinning) when the switch
    is off, the topology is unreadable, or the node has fewer than one CPU per builder."""
    if os.environ.get("IGN_PIN_BUILDERS", "0") != "1" or not hasattr(os, "sched_getaffinity"):
        return [set() for _ in range(workers)]
    try:
        allowed = os.sched_getaffinity(0)
        with open("/proc/self/stat") as f:
            cur = int(f.read().rsplit(")", 1)[1].split()[36])   # field 39: the CPU last run on
        node = set(allowed)
        for path in sorted(os.listdir("/sys/devices/system/node")):
            if not path.startswith("node"):
                continue
            cpus = set()
            with open("/sys/devices/system/node/%s/cpulist" % path) as f:
                for part in f.read().strip().split(","):
                    lo, _, hi = part.partition("-")
                    cpus.update(range(int(lo), int(hi or lo) + 1))
            if cur in cpus:
                node = cpus & set(allowed)
                break
    except (OSError, ValueError, IndexError):
        return [set() for _ in range(workers)]
    cand = sorted(node)
    # ranks of one node (torchrun's LOCAL_RANK) take disjoint slices; no pinning when they do not fit
    lr = int(os.environ.get("LOCAL_RANK", "0") or 0)
    per = 2 if len(cand) >= 2 * workers * (lr + 1) else 1 if len(cand) >= workers * (lr + 1) else 0
    if per == 0:
        return [set() for _ in range(workers)]
    base = lr * workers * per
    return [set(cand[base + per * i:base + per * i + per]) for i in range(workers)]


class BatchPrefetcher:
    """The training input pipeline overlapped with the GPU (the role of tf.data's
    ``map(num_parallel_calls)`` + ``prefetch``, GM:181-192).  ``workers`` threads take the next
    jobs of ``jobs`` (in order), turn each into (features, labels) with ``load`` (default: the job
    is that pair; with the native reader, ``NativeInput.load`` of a batch of sample ids) and run
    ``Trainer.prepare`` on it (the engine's host CSR build and copies, the training tables), while
    the main thread's step runs on the GPU.  At most ``depth`` batches are built ahead.  Iterating
    yields prepared (batch, labels) pairs in job order, for ``Trainer.train_prepared``; an
    exception in a worker is raised in the consumer at its position."""

    _END = object()

    def __init__(self, trainer: Trainer, jobs, depth: int = 2, workers: int = 1, load=None):
        import threading
        self.trainer = trainer
        self.jobs = iter(jobs)
        self.load = load
        self.lock = threading.Lock()          # the job iterator
        self.cv = threading.Condition()       # results by sequence number
        self.slots = threading.Semaphore(max(1, depth))
        self.results = {}
        self.issued = 0
        self.end = None                       # sequence number of the end of the jobs
        self.next_out = 0
        self.stop = threading.Event()
        cpus = builder_cpus(max(1, workers))
        self.threads = [threading.Thread(target=self._run, args=(c,), daemon=True) for c in cpus]
        for t in self.threads:
            t.start()

    def _run(self, cpus=frozenset()):
        if cpus:
            try:
                os.sched_setaffinity(0, cpus)   # this thread (Linux: pid 0 is the caller)
            except OSError:
                pass
        while True:
            while not self.slots.acquire(timeout=0.1):
                if self.stop.is_set():
                    return
            if self.stop.is_set():
                return
            with self.lock:
                if self.end is not None:
                    self.slots.release()
                    return
                k = self.issued
                try:
                    job = next(self.jobs)
                except StopIteration:
                    self.end = k
                    with self.cv:
                        self.cv.notify_all()
                    self.slots.release()
                    return
                except BaseException as e:
                    self.end = k + 1
                    job = e
                self.issued += 1
            try:
                if isinstance(job, BaseException):
                    raise job
                features, labels = self.load(job) if self.load is not None else job
                res = self.trainer.prepare(features, labels)
                # the gathered arrays are copied into the batch: drop them now, so that the native
                # reader's buffers go back to its pool before this worker's next gather
                del features, labels
            except BaseException as e:   # handed to the consumer
                res = e
            with self.cv:
                self.results[k] = res
                self.cv.notify_all()

    def __iter__(self):
        return self

    def __next__(self):
        with self.cv:
            while self.next_out not in self.results:
                if self.end is not None and self.next_out >= self.end:
                    raise StopIteration
                self.cv.wait(0.1)
            res = self.results.pop(self.next_out)
            self.next_out += 1
        self.slots.release()
        if isinstance(res, BaseException):
            raise res
        return res

    def close(self):
        self.stop.set()
        for t in self.threads:
            t.join()
        with self.cv:
            for res in self.results.values():
                if isinstance(res, tuple):
                    res[0].close()
            self.results.clear()
