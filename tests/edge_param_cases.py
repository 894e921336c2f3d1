"""Message-network models that read per-edge parameters (tests/test_gpu_edge_params.py and the CPU
pin of its oracle): {name: builder -> (desc, dims, graphs, labels, parameters)}.

Two NSFNET graphs (406 + 414 path-link pairs: 820 edges together, no multiple of a 256-thread
block), T = 2 so that a source's gradient is a sum over two MP instances, H = 32 on both entities
unless said.  S, D, E: hs_source, hs_dest, edge_params; the column of the edge_params slice in the
network's input rows [edges][din] and din, the rows' leading dimension:

  case              MP with the network         inputs      P   E at column   din   kernel form
  sum_p1_first      path -> link, sum           E S D       1   0             65    one column
  sum_p2_middle     path -> link, sum           S E D       2   32            66    one column
  sum_p3_last       path -> link, sum           D S E       3   64            67    one column
  sum_p4_first      path -> link, sum           E S D       4   0             68    four columns
  sum_p4_middle     path -> link, sum           S E D       4   32            68    four columns
  sum_p3_twice      path -> link, sum           E S E       3   0 and 35      38    one column, 35 % 4 != 0
  sum_p4_twice      path -> link, sum           E E D       4   0 and 4       40    four columns, twice
  ordered_p1_middle link -> path, ordered       S E D       1   32            65    one column
  ordered_mixed     tests/width_cases.py msgnet_ordered_mixed (T = 3): S (16) D (32) E, P = 2 at 48, din 50
  attention_p2_last path -> link, attention     D S E       2   64            66    one column
  two_mps_p2        path -> link, sum, twice    D E S       2   32            66    two sources, one adjacency

A slice listed twice reads the one buffer twice: both slices' gradients are added to it.  two_mps_p2
repeats the path -> link MP in its stage: both read adj_paths_links, each owns a parameter buffer and
an accumulator, and both networks go by one name, so the engine holds two weight tensors of that name
(set alike by Engine.set_params) where the oracle holds one: the oracle's gradient of that name is the
sum of the engine's two."""
import copy
import functools

import numpy as np

from ignnition_amd import model_examples, synthetic, workloads
from ignnition_amd.engine import MPPlan
from ignnition_amd.framework_operations import dimensions_of_sample
from ignnition_amd.json_operations import Model_information

T = 2
S, D, E = "hs_source", "hs_dest", "edge_params"


def _net(desc, stage, inputs, units, act):
    src = desc["message_passing"]["stages"][stage]["stage_mp"][0]["source_entities"][0]
    src["message"] = [{"type": "neural_network", "nn_name": "message_nn", "input": list(inputs)}]
    desc["neural_networks"].append({"nn_name": "message_nn", "nn_type": "feed_forward", "nn_architecture": [
        {"type_layer": "Dense", "units": u, "activation": act} for u in units]})
    return desc


def with_params(sample, adj, P, rng):
    """The sample with P parameters on every edge of adjacency ``adj``."""
    s = dict(sample)
    s[adj] = {d: [[x, [float(v) for v in rng.uniform(-1, 1, P)]] for x in xs] for d, xs in sample[adj].items()}
    return s


def _case(kind, inputs, P, seed, units=(32,), act="tanh", twice=False, ids=(0, 1)):
    def build():
        rng = np.random.default_rng(17)
        desc = model_examples.routenet(iterations=T)
        stage, adj = (0, "adj_links_paths") if kind == "ordered" else (1, "adj_paths_links")
        _net(desc, stage, inputs, units, act)
        if kind == "attention":
            desc["message_passing"]["stages"][1]["stage_mp"][0]["aggregation"] = {"type": "attention"}
        if twice:
            mps = desc["message_passing"]["stages"][1]["stage_mp"]
            mps.append(copy.deepcopy(mps[0]))
        samples = [with_params(synthetic.routenet_sample("nsfnet", g), adj, P, rng) for g in ids]
        dims = dimensions_of_sample(samples[0])
        mi = Model_information(copy.deepcopy(desc), dims)
        graphs, labels = workloads.graph_inputs(mi, samples)
        return desc, dims, graphs, labels, MPPlan.from_model_info(mi).init_params(seed, bias_scale=0.1)
    return build


def _ordered_mixed():
    from tests import width_cases
    desc, dims, _, _, graphs, labels, prm = width_cases.case_inputs("msgnet_ordered_mixed")
    return desc, dims, graphs, labels, prm


CASES = {
    "sum_p1_first": _case("sum", (E, S, D), 1, 6),
    "sum_p2_middle": _case("sum", (S, E, D), 2, 6),
    "sum_p3_last": _case("sum", (D, S, E), 3, 6),
    "sum_p4_first": _case("sum", (E, S, D), 4, 6),
    "sum_p4_middle": _case("sum", (S, E, D), 4, 6, units=(24, 32), act="selu"),
    "sum_p3_twice": _case("sum", (E, S, E), 3, 6),
    "sum_p4_twice": _case("sum", (E, E, D), 4, 6),
    "ordered_p1_middle": _case("ordered", (S, E, D), 1, 6),
    "ordered_mixed": _ordered_mixed,
    "attention_p2_last": _case("attention", (D, S, E), 2, 8),
    "two_mps_p2": _case("sum", (D, E, S), 2, 6, twice=True),
}
ADJ = {name: "adj_links_paths" if name.startswith("ordered") else "adj_paths_links" for name in CASES}
# (column of each edge_params slice, din): what the table above says, asserted against the plan
COLUMNS = {"sum_p1_first": ([0], 65), "sum_p2_middle": ([32], 66), "sum_p3_last": ([64], 67), "sum_p4_first": ([0], 68),
           "sum_p4_middle": ([32], 68), "sum_p3_twice": ([0, 35], 38), "sum_p4_twice": ([0, 4], 40),
           "ordered_p1_middle": ([32], 65), "ordered_mixed": ([48], 50), "attention_p2_last": ([64], 66),
           "two_mps_p2": ([32], 66)}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(desc, dims, graphs, labels, parameters) of a case, built once per session; read-only."""
    return CASES[name]()


def slice_columns(plan, adj):
    """([column of every edge_params slice], din) of the first network that reads ``adj``'s parameters."""
    for mp in plan.mps:
        for src, net in zip(mp["sources"], mp["nets"]):
            if net and E in net["inputs"] and plan.adj_slots[src[1]].adj == adj:
                width = {S: plan.hidden[src[0]], D: plan.hidden[mp["dst"]], E: net["param_dim"]}
                cols, col = [], 0
                for i in net["inputs"]:
                    if i == E:
                        cols.append(col)
                    col += width[i]
                return cols, col
    raise KeyError(adj)


def edge_values(graphs, adj):
    """[edges of the batch, P]: the graphs' params_<adj> stacked."""
    n = [len(np.asarray(g["src_" + adj]).reshape(-1)) for g in graphs]
    return np.concatenate([np.asarray(g["params_" + adj], np.float32).reshape(k, -1) for g, k in zip(graphs, n)])


def other_values(graphs, adj, seed):
    """The same graphs with every params_<adj> value drawn again (feature values kept)."""
    rng = np.random.default_rng(seed)
    out = []
    for g in graphs:
        g = dict(g)
        g["params_" + adj] = rng.uniform(-1, 1, np.asarray(g["params_" + adj]).shape).astype(np.float32)
        out.append(g)
    return out
