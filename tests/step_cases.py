"""Models for the gradient-after-an-update tests (tests/test_gpu_train_steps.py):
{name: (builder -> (desc, dims, graphs, labels, parameters P0), {switch: value})}.

Every case is one or two NSFNET graphs (synthetic_h64: one 1500-node synthetic graph), T = 2 or 3, and
takes one Adam step of rate LR (Keras defaults otherwise) from P0 to P1.  The step has to move every
gradient tensor by much more than the tolerance the gradients are held to, or a pack left at P0 could
hide inside it: the last column is the float64 oracle's smallest per-tensor

    ||g(P1) - g(P0)|| / ||g(P1)||      (TorchOracle at both; P1 = oracle.train_oracle.adam_step, as float32)

over the tensors with a non-zero gradient, which must exceed 10 * GTOL = 1e-3.

  case                        P0                        smallest ratio (tensor)
  routenet_h32 (+ _per_mp,    init_params(7, 0.1)       0.999 (link_update/recurrent_kernel)
    _f32, _variant5: the same model)
  routenet_h16                init_params(2, 0.2)       0.995 (path_update/bias)
  synthetic_h64               init_params(4, 0.1)       0.993 (node_update/bias)
  qsize                       init_params(7, 0.1)       0.995 (node_update/recurrent_kernel)
  rn_l16_p32                  width_cases (5, 0.1)      0.999 (path_update/kernel)
  concat2_l16_n32_p32         width_cases               0.993 (link_update/recurrent_kernel)
  concat1_ln16_p32            width_cases               0.990 (node_update/bias)
  msgnet_sum_l2               init_params(6, 0.1)       0.981 (path_update/bias)
  msgnet_ordered              init_params(6, 0.1)       0.998 (link_to_path_message_creation_0/layer_0_.../kernel)
  msgnet_edge_params          init_params(6, 0.1)       0.981 (path_to_link_message_creation_0/layer_0_.../bias)
  attention                   init_params(4, 0.1)       0.990 (link_update/bias)
  attention_over_msgnet       init_params(8, 0.1)       0.983 (attention/kernel2)
  convolution_tanh            init_params(4, 0.1)       1.02  (path_update/kernel)
  predict_odd_widths          predict_cases (3, 0.2)    0.912 (path_update/bias)
  predict_four_layer          predict_cases             0.328 (readout_model_0/predict_0/kernel)
  predict_nobias_hidden       predict_cases             0.998 (path_update/bias)
  readout_nn_pool_product     init_params(11, 0.1)      0.996 (path_update/bias)

(Adam's first step moves every weight by about LR in the direction of its gradient's sign, and these
networks' gradients at a Glorot initialisation are small and far from converged, so g(P1) is nearly
unrelated to g(P0).)
"""
import copy

import numpy as np

from ignnition_amd import model_examples, synthetic, workloads
from ignnition_amd.engine import MPPlan
from ignnition_amd.json_operations import Model_information

LR = 0.01            # the one Adam step's rate (iteration 0, beta_1 0.9, beta_2 0.999, epsilon 1e-7)

# every training switch that picks another pack of the cell or of the predict Dense layers
F32 = {"IGN_BWD_BF": "0", "IGN_TRAIN_SEQ_H16": "0", "IGN_TRAIN_DENSE_H16": "0", "IGN_TRAIN_DENSE_BF": "0",
       "IGN_TSGEMM_BF": "0"}


def _nsfnet(desc, seed, bias, qsize=False, ids=(0, 1)):
    _, dims, _ = workloads.model("qsize" if qsize else "routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, labels = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", g, qsize=qsize) for g in ids])
    return desc, dims, graphs, labels, MPPlan.from_model_info(mi).init_params(seed, bias_scale=bias)


def _routenet(hidden, seed, bias):
    return lambda: _nsfnet(model_examples.routenet(hidden=hidden, iterations=3), seed, bias)


def _qsize():
    return _nsfnet(model_examples.qsize(iterations=2), 7, 0.1, qsize=True)


def _synthetic():
    desc, dims, mi, graphs, labels = workloads.make_synthetic_inputs(n_nodes=1500, iterations=2, window=40)
    return desc, dims, graphs, [np.asarray(l, np.float32) for l in labels], \
        MPPlan.from_model_info(mi).init_params(4, bias_scale=0.1)


def _width(name):
    def build():
        from tests.width_cases import case_inputs
        desc, dims, _, _, graphs, labels, prm = case_inputs(name)
        return desc, dims, graphs, labels, prm
    return build


def _msgnet(inputs, units, act, ordered=False, l2=None):
    def build():
        from tests.test_gpu_training import _msg_net_case
        return _msg_net_case(inputs, units, act, ordered, l2)
    return build


def _attention_over_msgnet():
    from tests.test_gpu_training import _msg_net_case
    desc, dims, graphs, labels, _ = _msg_net_case(("hs_source", "hs_dest"), (32,), "tanh")
    desc["message_passing"]["stages"][1]["stage_mp"][0]["aggregation"] = {"type": "attention"}
    prm = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)).init_params(8, bias_scale=0.1)
    return desc, dims, graphs, labels, prm


def _aggregation(aggr):
    return lambda: _nsfnet(model_examples.routenet_aggregation(aggr, hidden=32, iterations=3), 4, 0.1)


def _predict(case):
    def build():
        from tests.predict_cases import forward_case
        desc, dims, _, graphs, labels, prm, _ = forward_case(case)
        return desc, dims, graphs, labels, prm
    return build


def _readout(case):
    def build():
        from oracle.dense_forward import DenseOracle
        from tests.readout_cases import READOUT_CASES
        ops, pin, nets = READOUT_CASES[case]
        desc, dims, graphs, _, prm = _nsfnet(model_examples.routenet_readout(ops, pin, nets, iterations=3), 11, 0.1)
        ora = DenseOracle(desc, dims, prm)
        rng = np.random.default_rng(5)   # labels shaped like each graph's predictions
        return desc, dims, graphs, [rng.normal(size=ora.forward_graph(g).size).astype(np.float32) for g in graphs], prm
    return build


_PAIR = ("hs_source", "hs_dest")

STEP_CASES = {
    "routenet_h32": (_routenet(32, 7, 0.1), {}),
    "routenet_h32_per_mp": (_routenet(32, 7, 0.1), {"IGN_RESIDENT_TRAIN": "0"}),
    "routenet_h32_f32": (_routenet(32, 7, 0.1), F32),
    "routenet_h32_variant5": (_routenet(32, 7, 0.1), {"IGN_READOUT_VARIANT": "5"}),
    "routenet_h16": (_routenet(16, 2, 0.2), {}),
    "synthetic_h64": (_synthetic, {}),
    "qsize": (_qsize, {}),
    "rn_l16_p32": (_width("rn_l16_p32"), {}),
    "concat2_l16_n32_p32": (_width("concat2_l16_n32_p32"), {}),
    "concat1_ln16_p32": (_width("concat1_ln16_p32"), {}),
    "msgnet_sum_l2": (_msgnet(_PAIR, (48, 32), "selu", l2=0.01), {}),
    "msgnet_ordered": (_msgnet(_PAIR, (32,), "tanh", ordered=True), {}),
    "msgnet_edge_params": (_msgnet(("hs_dest", "hs_source", "edge_params"), (32,), "tanh"), {}),
    "attention": (_aggregation({"type": "attention"}), {}),
    "attention_over_msgnet": (_attention_over_msgnet, {}),
    "convolution_tanh": (_aggregation({"type": "convolution", "activation_function": "tanh"}), {}),
    "predict_odd_widths": (_predict("odd_widths"), {}),
    "predict_four_layer": (_predict("four_layer"), {}),
    "predict_nobias_hidden": (_predict("nobias_hidden"), {}),
    "readout_nn_pool_product": (_readout("nn_pool_product"), {}),
}
ORACLE_ANCHORED = ["routenet_h32", "msgnet_sum_l2"]   # F's gradient at P1 also against float64 autograd at P1


def step_ratios(g0: dict, g1: dict) -> dict:
    """{tensor: ||g1 - g0|| / ||g1||} over the tensors whose gradient g1 is not zero."""
    out = {}
    for name, b in g1.items():
        b = np.asarray(b, np.float64)
        if np.linalg.norm(b) > 0:
            out[name] = float(np.linalg.norm(b - np.asarray(g0[name], np.float64)) / np.linalg.norm(b))
    return out
