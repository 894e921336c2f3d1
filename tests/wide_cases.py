"""Models with every entity 128 wide (gru_wide.hip) on the graphs of tests/shape_cases.py, for
tests/test_gpu_wide.py and tests/test_wide_plan.py.  T = 2, init_params(SEED, bias_scale=BIAS) as shape_cases.
P paths are the ordered update's rows (16 per workgroup), L links the sum update's (64 per workgroup)."""
import copy
import functools

import numpy as np

from ignnition_amd.engine import MPPlan
from ignnition_amd.json_operations import Model_information
from tests import shape_cases as sc
from tests.shape_cases import BIAS, G, SEED, _rand

HIDDEN, T = 128, sc.ITERATIONS


def _mixed(P, long):   # length 1, then ``long``, then a cycle through 1 .. long: a tile masks rows from step 1 on
    return tuple(([1, long] + [1 + (3 * p) % long for p in range(2, P)])[:P])


_P17, _QS = G(17, 65, _mixed(17, 12)), G(20, 6, _rand(20, 4, 22), N=17)
CASES = {   # name: (model, graphs)
    "p1_l1": ("routenet", (G(1, 1, (1,)),)),                     # both tiles almost empty
    "p16_l63": ("routenet", (G(16, 63, _mixed(16, 12)),)),       # a full ordered tile; one row short of a sum tile
    "p17_l65": ("routenet", (_P17,)),                            # one row past either tile
    "p33_l64": ("routenet", (G(33, 64, _mixed(33, 9)),)),        # a third workgroup of one row; a full sum tile
    "len_all_1": ("routenet", (G(24, 7, 1),)),                   # one step: the state tile's second buffer unused
    "idle2": ("routenet", (G(40, 15, _rand(40, 3, 6), idle_links=2),)),   # destinations without a message
    "hot70": ("routenet", (G(80, 4, _rand(80, 3, 12), hot=70),)),         # 70 messages: the segmented class elsewhere
    "qsize": ("qsize", (_QS,)),                                  # interleave, multi rows, two sum MPs
    "concat1": ("concat1", (_QS,)),                              # concat on axis 1
    "batch2": ("routenet", (_P17, G(24, 7, 1, seed=1))),         # two graphs in one batch
}
BIG_SUM = ["hot70"]   # a sum of >= 64 float32 terms: held to _ieee_tol
PER_GRAPH = ["batch2", "p17_l65"]


def model(kind, hidden=HIDDEN):
    """(description, dims): RouteNet, Q-size, or Q-size with its path stage as an axis-1 concat."""
    desc, dims = sc.model("routenet" if kind == "routenet" else "qsize", hidden, T)
    if kind == "concat1":
        mp = desc["message_passing"]["stages"][0]["stage_mp"][0]
        mp["aggregation"] = {"type": "concat", "concat_axis": 1}
        mp.pop("interleave_definition", None)
    return desc, dims


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(desc, dims, plan, graphs, parameters) of a case, built once per session."""
    kind, specs = CASES[name]
    desc, dims = model(kind)
    graphs = [sc.graph(g, "routenet" if kind == "routenet" else "qsize") for g in specs]
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    return desc, dims, plan, graphs, plan.init_params(SEED, bias_scale=BIAS)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle's (predictions, {entity: final states over the batch}); callers do not modify them."""
    from oracle.dense_forward import DenseOracle
    desc, dims, plan, graphs, prm = case_inputs(name)
    ora = DenseOracle(desc, dims, prm)
    finals = [ora.final_states(g) for g in graphs]
    pred = np.concatenate([ora._readout(st, g).reshape(-1) for st, g in zip(finals, graphs)])
    states = {e: np.concatenate([st[e] for st in finals], axis=0) for e in plan.entities}
    return pred, states
