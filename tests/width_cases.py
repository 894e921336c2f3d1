"""Models whose entities do not share one hidden_state_dimension, and entity features of more than one
column, shared by the GPU parity / gradient tests (tests/test_gpu_widths.py) and the CPU plan-lowering
and C++-restatement tests: {name: builder -> (desc, dims, samples)}.

Samples are two NSFNET graphs (synthetic.routenet_sample, ids 0 and 1), T = 2 or 3; ``*_big`` swaps the
second one for Q-size synth50 graph 90, whose nodes carry 49-420 messages (the graph of
test_segmented_sum_rule_is_per_destination).  A wide feature is filled from a seeded numpy generator,
uniform in [-1, 1), and uses normalization "None".

Which kernels a case reaches (DIN = message width, H = destination width):

  rn_l16_p32                the ordered update's projected table from 16-wide rows (project<16,32>, dW [16][96],
                            dx [rows][16]), the sum update / backward at <32,16>, the readout at din 32
  rn_l32_p16                project<32,16>, sum_gru<16,32> / sum_gru_bwd<16,32>, the readout at din 16
  qs_ln16_p32 qs_ln32_p16   the interleave of two sources and two sum MPs, link = node != path
  qs_ln32_p16_big           sum_seg<16> (default) and sum_win<16> (IGN_SUM_WINDOW=1) feeding a 32-wide cell
  concat2_l16_n32_p32       axis-2 concat, slices 16 | 32 (DIN 48, slice offsets 0 and 16)
  concat2_l32_n16_p16       slices 32 | 16 (offset 32 in front of a 16-wide slice), H 16
  concat1_ln16_p32          axis-1 concat, link = node = 16 into path 32
  msgnet_sum_mixed          a message network on hs_source (32) | hs_dest (16): 48 columns, units (24, 16)
  msgnet_ordered_mixed      the ordered form, hs_source (16) | hs_dest (32) | edge_params (2): 50 columns padded
                            to 64, units (32,)
  feat_resident_rn          all H 32, link F = 3 + 2 (two features), path F = 7: the resident forward
  feat_resident_qs          Q-size, all H 32, link F 5, node F 2, path F 32 (no zero padding): resident, union
                            rows with two different feature widths
  feat_batched_h16          RouteNet at H 16, link F 16 (full width), path F 6: init_state4<4>
  rn_l16_p32_feat           rn_l16_p32 with link F 13 and path F 4
"""
import copy
import functools

import numpy as np

from ignnition_amd import model_examples, synthetic, workloads
from ignnition_amd.engine import MPPlan
from ignnition_amd.framework_operations import dimensions_of_sample
from ignnition_amd.json_operations import Model_information

SEED, BIAS = 5, 0.1          # init_params(SEED, bias_scale=BIAS)
BIG = ("synth50", 90)        # a Q-size graph with destinations of >= 64 messages


def _samples(qsize=False, big=False):
    s = [synthetic.routenet_sample("nsfnet", g, qsize=qsize) for g in range(2)]
    if big:
        s[1] = synthetic.routenet_sample(BIG[0], BIG[1], qsize=qsize)
    return s


def _set_widths(desc, **hidden):
    for e in desc["entities"]:
        e["hidden_state_dimension"] = hidden[e["name"]]
    return desc


def _set_features(desc, samples, seed, features):
    """Entity ``name``'s features become ``features[name]`` = [(feature name, columns), ...], each
    [rows][columns] in the samples (the list-of-lists layout dimensions_of_sample reads, FO:68-87)."""
    rng = np.random.default_rng(seed)
    for e in desc["entities"]:
        if e["name"] not in features:
            continue
        e["features"] = [{"name": f, "normalization": "None"} for f, _ in features[e["name"]]]
        for s in samples:
            rows = sum(1 for v in s["entities"].values() if v == e["name"])
            for f, cols in features[e["name"]]:
                s[f] = rng.uniform(-1, 1, (rows, cols)).round(6).tolist()
    return desc


def _routenet(link, path, iterations=3, features=None):
    def build():
        samples = _samples()
        desc = _set_widths(model_examples.routenet(iterations=iterations), link=link, path=path)
        _set_features(desc, samples, 11, features or {})
        return desc, dimensions_of_sample(samples[0]), samples
    return build


def _qsize(link, path, node, iterations=2, big=False, aggregation=None, features=None):
    def build():
        samples = _samples(qsize=True, big=big)
        desc = (model_examples.qsize_aggregation(aggregation, iterations=iterations) if aggregation
                else model_examples.qsize(iterations=iterations))
        _set_widths(desc, link=link, path=path, node=node)
        _set_features(desc, samples, 12, features or {})
        return desc, dimensions_of_sample(samples[0]), samples
    return build


def _msgnet_sum():
    samples = _samples()
    desc = model_examples.routenet_message_net(inputs=("hs_source", "hs_dest"), units=(24, 16), activation="selu",
                                               iterations=3)
    _set_widths(desc, link=16, path=32)
    return desc, dimensions_of_sample(samples[0]), samples


def _msgnet_ordered():
    rng = np.random.default_rng(13)
    samples = _samples()
    for s in samples:   # two edge parameters on every link -> path edge
        s["adj_links_paths"] = {p: [[l, [float(rng.uniform(0, 1)), float(rng.uniform(-1, 1))]] for l in ls]
                                for p, ls in s["adj_links_paths"].items()}
    desc = _set_widths(model_examples.routenet(iterations=3), link=16, path=32)
    src = desc["message_passing"]["stages"][0]["stage_mp"][0]["source_entities"][0]
    src["message"] = [{"type": "neural_network", "nn_name": "message_nn",
                       "input": ["hs_source", "hs_dest", "edge_params"]}]
    desc["neural_networks"].append({"nn_name": "message_nn", "nn_type": "feed_forward", "nn_architecture": [
        {"type_layer": "Dense", "units": 32, "activation": "tanh"}]})
    return desc, dimensions_of_sample(samples[0]), samples


_CONCAT1, _CONCAT2 = {"type": "concat", "concat_axis": 1}, {"type": "concat", "concat_axis": 2}

WIDTH_CASES = {
    "rn_l16_p32": _routenet(16, 32),
    "rn_l32_p16": _routenet(32, 16),
    "qs_ln16_p32": _qsize(16, 32, 16),
    "qs_ln32_p16": _qsize(32, 16, 32),
    "qs_ln32_p16_big": _qsize(32, 16, 32, big=True),
    "concat2_l16_n32_p32": _qsize(16, 32, 32, iterations=3, aggregation=_CONCAT2),
    "concat2_l32_n16_p16": _qsize(32, 16, 16, iterations=3, aggregation=_CONCAT2),
    "concat1_ln16_p32": _qsize(16, 32, 16, iterations=3, aggregation=_CONCAT1),
    "msgnet_sum_mixed": _msgnet_sum,
    "msgnet_ordered_mixed": _msgnet_ordered,
}
_F = {
    "feat_resident_rn": {"link": [("link_capacity", 3), ("link_load", 2)], "path": [("traffic", 7)]},
    "feat_resident_qs": {"link": [("link_capacity", 5)], "node": [("queue_sizes", 2)], "path": [("traffic", 32)]},
    "feat_batched_h16": {"link": [("link_capacity", 16)], "path": [("traffic", 6)]},
    "rn_l16_p32_feat": {"link": [("link_capacity", 13)], "path": [("traffic", 4)]},
}
FEATURE_CASES = {
    "feat_resident_rn": _routenet(32, 32, features=_F["feat_resident_rn"]),
    "feat_resident_qs": _qsize(32, 32, 32, iterations=3, features=_F["feat_resident_qs"]),
    "feat_batched_h16": _routenet(16, 16, features=_F["feat_batched_h16"]),
    "rn_l16_p32_feat": _routenet(16, 32, features=_F["rn_l16_p32_feat"]),
}
CASES = dict(WIDTH_CASES, **FEATURE_CASES)

RESIDENT = ["feat_resident_rn", "feat_resident_qs"]     # one mp_resident launch per forward; every other case: none
ROUTENET_WIDTHS = ["rn_l16_p32", "rn_l32_p16"]
QSIZE_WIDTHS = ["qs_ln16_p32", "qs_ln32_p16", "qs_ln32_p16_big"]
BIG_SUM = ["qs_ln32_p16_big"]                            # held to _ieee_tol: a sum of >= 64 float32 terms


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(desc, dims, mi, plan, graphs, labels, parameters) of a case, built once per session."""
    desc, dims, samples = CASES[name]()
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, labels = workloads.graph_inputs(mi, samples)
    plan = MPPlan.from_model_info(mi)
    return desc, dims, mi, plan, graphs, labels, plan.init_params(SEED, bias_scale=BIAS)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle's (predictions, {entity: final states over the batch}), read-only."""
    from oracle.dense_forward import DenseOracle
    desc, dims, _, plan, graphs, _, prm = case_inputs(name)
    ora = DenseOracle(desc, dims, prm)
    finals = [ora.final_states(g) for g in graphs]
    pred = np.concatenate([ora._readout(st, g).reshape(-1) for st, g in zip(finals, graphs)])
    states = {e: np.concatenate([st[e] for st in finals], axis=0) for e in plan.entities}
    for a in [pred] + list(states.values()):
        a.setflags(write=False)
    return pred, states
