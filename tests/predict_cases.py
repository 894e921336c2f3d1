"""Predict-network cases (the Dense stack of the readout's predict operation, GM:612-629) shared by
the forward parity, the gradient and the plan-lowering tests:
{name: [(units, activation, extra Dense options), ...]}.

Which kernels a case reaches (readout.cpp's readout_fused for the fused launch, from engine.cpp's
readout() in inference and, with the SAVE form, from train.cpp's ign_forward_train_end; else
engine.cpp's layer walk in inference and dense_stack.cpp's dense_stack_forward in training, and its
dense_stack_backward called by ign_backward_begin):

  relu tanh sigmoid linear selu   256 a, 256 a, 1: the fused kernels' five ACT instantiations (readout3,
                                  readout_bf, readout_h16 with and without SAVE, readout_h32); act' of the layer
                                  below in dense_h16_t / dense_bf_t / row_gemm_t and in the on-the-fly output rows
  sigmoid_out relu_out            act_apply(act3) in the fused kernels; launch_act_bwd on a non-linear output
  mixed                           act1 != act2: one launch_dense_generic per layer (inference); dense_h16 /
                                  dense_bf / dense_fwd per layer (training)
  nobias_hidden                   the fused path is refused; no bias gradient for layer 1
  nobias_out                      stays fused with b3 == nullptr
  one_layer                       L = 1: the M == 1 dot kernel; the backward with l == 0 only
  two_layer                       the outer-row fusion with the layer below at l = 0 (K = 64)
  four_layer                      the per-layer kernel choice: 32 -> 128 and 128 -> 256 on dense_h16 / dense_bf,
                                  256 -> 32 on dense_fwd_kernel, 32 -> 1 on the dot kernel
  odd_widths                      dense_generic, row_gemm_t_generic, d.in % 4 != 0 (no outer-row fusion)
  out3                            out_units > 1: not fused, predictions laid out [P][3]
  sat_*                           layers 1 and 2 (kernel and bias) x SATURATED[name] after init_params: saturated
                                  tanh / sigmoid, selu's deep negative arm, the layer-2 fp16 scale bound
"""
import copy
import functools

import numpy as np

from ignnition_amd import model_examples, synthetic, workloads
from ignnition_amd.engine import MPPlan
from ignnition_amd.json_operations import Model_information

_R1, _R3 = {"kernel_regularizer": 0.1}, {"kernel_regularizer": 0.01}   # model_examples._READOUT's
_NB = {"use_bias": False}


def _three(a1, a2=None, out="None", o1=_R1, o2=_R1, o3=_R3):
    return [(256, a1, dict(o1)), (256, a2 or a1, dict(o2)), (1, out, dict(o3))]


PREDICT_CASES = {
    "relu": _three("relu"),
    "tanh": _three("tanh"),
    "sigmoid": _three("sigmoid"),
    "linear": _three("linear"),
    "selu": _three("selu"),
    "sigmoid_out": _three("selu", out="sigmoid"),
    "relu_out": _three("selu", out="relu"),
    "mixed": _three("relu", "tanh"),
    "nobias_hidden": _three("selu", o1=dict(_R1, **_NB)),
    "nobias_out": _three("selu", o3=dict(_R3, **_NB)),
    "one_layer": [(1, "None", dict(_R3))],
    "two_layer": [(64, "relu", dict(_R1)), (1, "None", {})],
    "four_layer": [(128, "selu", dict(_R1)), (256, "tanh", {}), (32, "sigmoid", dict(_R3)), (1, "sigmoid", {})],
    "odd_widths": [(100, "tanh", dict(_R1)), (7, "selu", {}), (1, "None", dict(_R3))],
    "out3": [(256, "selu", dict(_R1)), (256, "selu", dict(_R1)), (3, "None", dict(_R3))],
    "sat_relu": _three("relu"),
    "sat_selu": _three("selu"),
    "sat_tanh": _three("tanh"),
    "sat_sigmoid": _three("sigmoid"),
}
# the factor on layers 1 and 2 (kernel and bias) after init_params.  x16 leaves 21-28 % of the float64
# oracle's layer-1 tanh activations and 3-7 % of its sigmoid activations within 1e-3 of an asymptote
# (H = 32 / 64); x64 puts 75-79 % and 59-61 % there
SATURATED = {"sat_relu": 16.0, "sat_selu": 16.0, "sat_tanh": 64.0, "sat_sigmoid": 64.0}
FUSED = ["relu", "tanh", "sigmoid", "linear", "selu", "sigmoid_out", "relu_out", "nobias_out"]
UNFUSED = ["mixed", "nobias_hidden", "one_layer", "two_layer", "four_layer", "odd_widths", "out3"]
SEED = 3          # init_params(SEED, bias_scale=BIAS)
# relu_out at seed 3: every oracle output positive at H = 16 and 32, every one zero at H = 64; at seed 12
# 100 % / 80 % / 66 % are positive (H = 16 / 32 / 64), so both arms of the output relu run at 32 and 64
SEEDS = {"relu_out": 12}
BIAS = 0.2
# predict_inputs(*WIDE): the plain-sum model at DIN = H = 64, where IGN_SUM_VARIANT selects among three
# sum kernels (3: f32 MFMA, 7: split-bf16, 8: split-fp16, which saves nothing and so never trains)
WIDE = ("selu", 64)


def layer_name(i):
    return "predict_%d" % i


def predict_model(case, hidden=32, ops=(), predict_input=("path",)):
    """model_examples.routenet(hidden, iterations=3) with PREDICT_CASES[case] as the readout_model
    architecture (layers named predict_<i>: parameters readout_model_<k>/predict_<i>/kernel), reading
    ``predict_input`` after the readout operations ``ops``."""
    desc = model_examples.routenet_readout(list(ops), list(predict_input), None, hidden=hidden, iterations=3)
    arch = [dict({"type_layer": "Dense", "name": layer_name(i), "units": u, "activation": a}, **extra)
            for i, (u, a, extra) in enumerate(PREDICT_CASES[case])]
    for net in desc["neural_networks"]:
        if net["nn_name"] == "readout_model":
            net["nn_architecture"] = arch
    return desc


def predict_inputs(case, hidden=32, n_graphs=2, ops=(), predict_input=("path",)):
    """(desc, dims, plan, graphs, labels, parameters): NSFNET samples 0 .. n_graphs - 1 (two samples: 364
    path rows, two full 128-row groups of readout_h16 and a partial one ending in a 12-row tile)."""
    desc = predict_model(case, hidden, ops, predict_input)
    _, dims, _ = workloads.model("routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, labels = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", g) for g in range(n_graphs)])
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(SEEDS.get(case, SEED), bias_scale=BIAS)
    if case in SATURATED:
        pre = "readout_model_%d/" % len(ops)
        for i in (0, 1):
            for t in ("kernel", "bias"):
                k = pre + layer_name(i) + "/" + t
                prm[k] = prm[k] * np.float32(SATURATED[case])
    return desc, dims, plan, graphs, labels, prm


@functools.lru_cache(maxsize=None)
def forward_case(case, hidden=32):
    """predict_inputs(case, hidden) and the float64 oracle's predictions, computed once per session
    and shared (read-only) by the tests."""
    from oracle.dense_forward import DenseOracle
    desc, dims, plan, graphs, labels, prm = predict_inputs(case, hidden)
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    ref.setflags(write=False)
    return desc, dims, plan, graphs, labels, prm, ref


def layer1_activations(case, hidden=32):
    """The float64 oracle's layer-1 activations [P][units]: the same model cut after its first Dense."""
    from oracle.dense_forward import DenseOracle
    desc, dims, _, graphs, _, prm, _ = forward_case(case, hidden)
    cut = copy.deepcopy(desc)
    for net in cut["neural_networks"]:
        if net["nn_name"] == "readout_model":
            net["nn_architecture"] = net["nn_architecture"][:1]
    units = PREDICT_CASES[case][0][0]
    return DenseOracle(cut, dims, prm).forward(graphs).reshape(-1, units)
