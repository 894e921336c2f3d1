"""GRU cells with the GRUCell keys the engine lowers beside ``units`` (activation, recurrent_activation,
use_bias, reset_after; ign_plan_set_cell_options), shared by tests/test_gru_options_host.py (CPU) and
tests/test_gpu_gru_options.py: {name: builder -> (desc, dims, samples)}, and the two oracles with a
Keras GRUCell restatement that takes the four options.

Samples are two NSFNET graphs (synthetic.routenet_sample, ids 0 and 1), T = 2, as tests/width_cases.py
builds its own: no entity's row count is a multiple of 16, so partial tiles and masked steps are reached.

The oracles (oracle/ is not edited): CellDenseOracle / CellTorchOracle subclass DenseOracle / TorchOracle,
override ``_cell`` (the cell's tensors; no bias tensor under use_bias false) and step it with
``gru_cell_np`` / ``gru_cell_torch`` in place of the parents' module-level gru_cell for the duration of
one message passing.  With default options the restatement is the parents' arithmetic operation for
operation (tests/test_gru_options_host.py checks the bits).

Which kernels a case reaches (gru_cell.hip):

  rn_hard_sigmoid rn_relu   seq_gru_cell<32> / sum_gru_cell<32,32,0> with another gate / candidate function
  rn_no_bias                the zero bias block, no bias tensor in the layout or the gradient
  rn_v1                     reset_after false: the candidate's sweep on r * h, bias [3H], dU from two contractions
  rn_all_four               the four together
  rn_v1_l16_p32             reset_after false at project<16,32>, seq_gru_cell<32>, sum_gru_cell<32,16>
  rn_v1_h64                 seq_gru_cell<64>, sum_gru_cell<64,64> with W / U in LDS
  qs_path_v1                Q-size interleave: a reset_after false path cell beside default link / node cells
                            (two cell kinds in one plan; the resident forward must report ineligible)
  rn_attention_v1 rn_convolution_v1   sum_gru_cell<32,32,1> / <32,32,2> on the link cell
  concat2_no_bias           axis-2 concat into a use_bias false cell (the hoisted per-slice x.W)
"""
import contextlib
import copy
import functools

import numpy as np
import torch

import oracle.dense_forward as dense
import oracle.train_oracle as train
from ignnition_amd import model_examples, synthetic, workloads
from ignnition_amd.engine import GRU_OPTION_DEFAULTS, MPPlan
from ignnition_amd.framework_operations import dimensions_of_sample
from ignnition_amd.json_operations import Model_information
from tests import activation_cases as ac

SEED, BIAS = 5, 0.1          # init_params(SEED, bias_scale=BIAS)
T = 2


def _samples(qsize=False):
    return [synthetic.routenet_sample("nsfnet", g, qsize=qsize) for g in range(2)]


def _gru(desc, name="recurrent1"):
    return [n for n in desc["neural_networks"] if n["nn_name"] == name][0]


def _routenet(options, hidden=32, widths=None, aggregation=None):
    def build():
        samples = _samples()
        desc = (model_examples.routenet_aggregation(aggregation, hidden=hidden, iterations=T) if aggregation
                else model_examples.routenet(hidden=hidden, iterations=T))
        for e in desc["entities"]:
            e["hidden_state_dimension"] = (widths or {}).get(e["name"], hidden)
        _gru(desc).update(options)
        return desc, dimensions_of_sample(samples[0]), samples
    return build


def _qsize_path(options):
    """Q-size whose path cell alone takes ``options`` (a network of its own); link and node cells: defaults."""
    def build():
        samples = _samples(qsize=True)
        desc = model_examples.qsize(iterations=T)
        desc["neural_networks"].append(dict(_gru(desc), nn_name="recurrent_path", **options))
        desc["message_passing"]["stages"][0]["stage_mp"][0]["update"]["nn_name"] = "recurrent_path"
        return desc, dimensions_of_sample(samples[0]), samples
    return build


def _concat2(options):
    def build():
        samples = _samples(qsize=True)
        desc = model_examples.qsize_aggregation({"type": "concat", "concat_axis": 2}, iterations=T)
        _gru(desc).update(options)
        return desc, dimensions_of_sample(samples[0]), samples
    return build


V1 = {"reset_after": False}
HS, RELU, NO_BIAS = {"recurrent_activation": "hard_sigmoid"}, {"activation": "relu"}, {"use_bias": False}
ALL_FOUR = dict(HS, **RELU, **NO_BIAS, **V1)
CASES = {
    "rn_hard_sigmoid": _routenet(HS),
    "rn_relu": _routenet(RELU),
    "rn_no_bias": _routenet(NO_BIAS),
    "rn_v1": _routenet(V1),
    "rn_all_four": _routenet(ALL_FOUR),
    "rn_v1_l16_p32": _routenet(V1, widths={"link": 16, "path": 32}),
    "rn_v1_h64": _routenet(V1, hidden=64),
    "qs_path_v1": _qsize_path(V1),
    "rn_attention_v1": _routenet(V1, aggregation={"type": "attention"}),
    "rn_convolution_v1": _routenet(V1, aggregation={"type": "convolution"}),
    "concat2_no_bias": _concat2(NO_BIAS),
}
# the same models with every option written out at its Keras default: default cells
DEFAULTS_WRITTEN = {"routenet": (_routenet({}), _routenet(dict(GRU_OPTION_DEFAULTS))),
                    "qsize": (_qsize_path({}), _qsize_path(dict(GRU_OPTION_DEFAULTS)))}


# ---------------------------------------------------------------------------------------------
# the cell
def cell_options(desc, dst):
    """The four options of entity ``dst``'s cell: the keys of its first MP's update dict and network
    (JO:287-291), the Keras GRUCell defaults for the absent ones."""
    nets = {n["nn_name"]: n for n in desc["neural_networks"]}
    for stage in desc["message_passing"]["stages"]:
        for mp in stage["stage_mp"]:
            if mp["destination_entity"] == dst:
                keys = dict(nets[mp["update"]["nn_name"]], **mp["update"])
                return {k: keys.get(k, v) for k, v in GRU_OPTION_DEFAULTS.items()}
    raise KeyError(dst)


def _act_np(x, name):
    if name == "sigmoid":                      # the parent oracle's own form, to the bit
        return 1 / (1 + np.exp(-x))
    return ac.act_np(x, name) if name in ac.CODES else dense._act(x, name)


def _act_torch(x, name):
    return ac.act_torch(x, name) if name in ac.CODES else train._act(x, name)


def _gru_cell(x, h, kernel, recurrent_kernel, bias, o, act):
    """tf.keras.layers.GRUCell (TF 2.x) one step, gates z, r, h.  bias: [2][3H] (reset_after), [3H], or
    None (use_bias false).  numpy or torch by ``act``."""
    H = h.shape[1]
    if o["reset_after"]:
        mx = x @ kernel
        mh = h @ recurrent_kernel
        if bias is not None:
            mx = mx + bias[0]
            mh = mh + bias[1]
        z = act(mx[:, :H] + mh[:, :H], o["recurrent_activation"])
        r = act(mx[:, H:2 * H] + mh[:, H:2 * H], o["recurrent_activation"])
        hh = act(mx[:, 2 * H:] + r * mh[:, 2 * H:], o["activation"])
    else:
        mx = x @ kernel
        if bias is not None:
            mx = mx + bias
        z = act(mx[:, :H] + h @ recurrent_kernel[:, :H], o["recurrent_activation"])
        r = act(mx[:, H:2 * H] + h @ recurrent_kernel[:, H:2 * H], o["recurrent_activation"])
        hh = act(mx[:, 2 * H:] + (r * h) @ recurrent_kernel[:, 2 * H:], o["activation"])
    return z * h + (1 - z) * hh


def gru_cell_np(x, h, kernel, recurrent_kernel, bias, o):
    with np.errstate(over="ignore"):
        return _gru_cell(x, h, kernel, recurrent_kernel, bias, o, _act_np)


def gru_cell_torch(x, h, kernel, recurrent_kernel, bias, o):
    return _gru_cell(x, h, kernel, recurrent_kernel, bias, o, _act_torch)


class _CellMixin:
    """``_cell`` hands out the cell's tensors and remembers whose they are; the message passing that asked
    steps them with the restatement above instead of the module's default-only gru_cell."""
    _module = None
    _step = None

    def _cell(self, dst):
        pre = dst + "_update/"
        self._options = cell_options(self.d, dst)
        return self.p[pre + "kernel"], self.p[pre + "recurrent_kernel"], self.p.get(pre + "bias")

    def _message_passing(self, mp, state, x):
        step = type(self)._step
        with _patched(self._module, "gru_cell", lambda xx, h, k, rk, b: step(xx, h, k, rk, b, self._options)):
            return super()._message_passing(mp, state, x)


@contextlib.contextmanager
def _patched(module, name, value):
    old = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, old)


class CellDenseOracle(_CellMixin, dense.DenseOracle):
    _module = dense
    _step = staticmethod(gru_cell_np)


class CellTorchOracle(_CellMixin, train.TorchOracle):
    _module = train
    _step = staticmethod(gru_cell_torch)


# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(desc, dims, mi, plan, graphs, labels, parameters) of a case, built once per session."""
    desc, dims, samples = CASES[name]()
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, labels = workloads.graph_inputs(mi, samples)
    plan = MPPlan.from_model_info(mi)
    return desc, dims, mi, plan, graphs, labels, plan.init_params(SEED, bias_scale=BIAS)


def _reference(name, dtype):
    desc, dims, _, plan, graphs, _, prm = case_inputs(name)
    ora = CellDenseOracle(desc, dims, prm, dtype=dtype)
    finals = [ora.final_states(g) for g in graphs]
    pred = np.concatenate([ora._readout(st, g).reshape(-1) for st, g in zip(finals, graphs)])
    states = {e: np.concatenate([st[e] for st in finals], axis=0) for e in plan.entities}
    for a in [pred] + list(states.values()):
        a.setflags(write=False)
    return pred, states


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle's (predictions, {entity: final states over the batch}), read-only."""
    return _reference(name, np.float64)


@functools.lru_cache(maxsize=None)
def float32_error(name):
    """The maximum scaled error (|a - b| / max(1, |b|)) of a float32 numpy run of the same restatement
    against its float64 run, over the predictions and every entity's final states."""
    p32, s32 = _reference(name, np.float32)
    p64, s64 = reference(name)
    err = lambda a, b: float((np.abs(np.asarray(a, np.float64) - b) / np.maximum(1.0, np.abs(b))).max())
    return max([err(p32, p64)] + [err(s32[e], s64[e]) for e in s64])


@functools.lru_cache(maxsize=None)
def autograd(name):
    """CellTorchOracle.loss_and_grads of the case: (loss, l2 term, {tensor: gradient}, predictions)."""
    desc, dims, _, _, graphs, labels, prm = case_inputs(name)
    return CellTorchOracle(desc, dims, prm).loss_and_grads(graphs, labels)
