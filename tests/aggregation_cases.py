"""The attention, convolution and concat MPs on graphs built at the routing level (tests/shape_cases.py's
builders), so that a test chooses what their kernels tile over: the cells of an attention group, the
groups of a block, a destination's in-degree, the destination rows.

Attention (AUX:287-343): the scores are scattered into a dense [destinations, positions] table per graph
and the softmax runs over the destinations of each position, so a (graph, position) pair is one group,
a (destination, position) pair that holds a message one cell, and a destination of the graph without a
message at that position an empty cell that scores 0.  The engine runs one wave per group (four groups
per block, lanes striding the cells by 64).
  RouteNet path -> link: the destination is the link, the position the message's seq_path_link (its
  index in the link's list), so group q holds the links of more than q messages.
  Q-size {link, node} -> path: the destination is the path; a path of length k holds its link messages
  at positions 0 .. k - 1 and its node messages at k .. 2k - 1 (the second source's positions are offset
  by its own count, GM:539-540).

Two cases of the issue cannot be built as it words them, and stand here in the nearest form that can:
  a graph whose only links are idle has no path -> link message at all, so it has no group (and the
  reference takes reduce_max of an empty seq).  The group without a cell next to live groups of the
  same block (attn_softmax_kernel's c0 == c1 return) is reached by a skipped position instead
  (att_hole); the idle link next to live links (group_empty > 0 in every group) is att_idle.

CASES is the table tests/test_gpu_aggregations.py sweeps and tests/test_aggregation_cases.py checks
against the arrays: T = 2, init_params(SEED, bias_scale=BIAS), a few hundred rows per graph at most.
No GPU is needed here."""
import collections
import copy
import functools

import numpy as np

from ignnition_amd import model_examples
from ignnition_amd.engine import MPPlan
from ignnition_amd.json_operations import Model_information
from tests import shape_cases as sc
from tests.shape_cases import G, _one_long, _rand

ATT = (("type", "attention"),)
CAT1 = (("type", "concat"), ("concat_axis", 1))
CAT2 = (("type", "concat"), ("concat_axis", 2))
ATTN_KERNEL = "attention/attn_kernel"


def CONV(act=None):
    return (("type", "convolution"),) + ((("activation_function", act),) if act else ())


# graphs: G(...) specs; scale: ((parameter name, factor), ...) applied after init_params; grads: the case is
# also a gradient case; cells / empty: per graph, the stated cell count and empty-cell count of every
# group in position order; mod4: n_groups % 4 of the batch; dup: some cell holds two messages;
# deg0: link 0's stated in-degree; idle: the stated destination row without a message
Case = collections.namedtuple("Case", "kind aggr hidden graphs scale grads cells empty mod4 dup deg0 idle")


def _c(kind, aggr, *graphs, hidden=32, scale=(), grads=True, cells=None, empty=None, mod4=None, dup=False, deg0=None,
       idle=None):
    return Case(kind, aggr, hidden, tuple(graphs), tuple(scale), grads, cells, empty, mod4, dup, deg0, idle)


_HOT65 = G(68, 65, 1, hot=3)       # 65 links: link 0 crossed 3 times, link 1 twice, every other link once
_HOT129 = G(134, 129, 1, hot=4)    # 129 links: link 0 crossed 4 times, links 1 and 2 twice
_ONE = G(3, 1, 1)                  # one link crossed by three paths: three groups of one cell
_PAIR = G(2, 2, 2, seed=1)         # two links, both crossed by both paths: two groups of two cells
_HOLE = G(2, 2, 2, link_positions=((0, (0, 2)), (1, (0, 2))))   # no link fills position 1
_DUP = G(3, 2, (2, 2, 1), link_positions=((0, (0, 0, 1)),))      # link 0: two messages at position 0
_IDLE = G(6, 3, 2, idle_links=1)   # three links of four messages and an idle one: an empty cell in every group


def _q(P, at, **kw):
    """Q-size: P paths of length 1 and path ``at`` of length 3, over 4 links and 4 nodes: groups 0 and 1
    hold every path, groups 2 .. 5 the long path and P - 1 empty cells."""
    return G(P, 4, _one_long(P, 3, at), N=4, **kw)


def _qcells(P):
    return ((P, P, 1, 1, 1, 1),), ((0, 0, P - 1, P - 1, P - 1, P - 1),)


def _qatt(P, at, **kw):
    cells, empty = _qcells(P)
    return _c("qsize", ATT, _q(P, at), cells=cells, empty=empty, mod4=2, **kw)


CASES = {
    # attention, RouteNet path -> link: the cells of group 0 are the L links
    "att_l1": _c("routenet", ATT, _ONE, cells=((1, 1, 1),), empty=((0, 0, 0),), mod4=3),   # groups of one cell
    "att_l63": _c("routenet", ATT, G(63, 63, 1), cells=((63,),), empty=((0,),), mod4=1),    # one cell short of the wave
    "att_l64": _c("routenet", ATT, G(64, 64, 1), cells=((64,),), empty=((0,),), mod4=1),    # every lane, one trip
    "att_l65": _c("routenet", ATT, _HOT65, cells=((65, 2, 1),), empty=((0, 63, 64),), mod4=3),   # lane 0's second trip
    "att_l129": _c("routenet", ATT, _HOT129, cells=((129, 3, 1, 1),), empty=((0, 126, 128, 128),), mod4=0),   # a third trip
    # n_groups at the edges of the four-group block
    "att_b5": _c("routenet", ATT, _ONE, _PAIR, cells=((1, 1, 1), (2, 2)), empty=((0, 0, 0), (0, 0)), mod4=1),
    "att_b7": _c("routenet", ATT, _ONE, _PAIR, G(4, 2, 1, seed=2), cells=((1, 1, 1), (2, 2), (2, 2)),
                 empty=((0, 0, 0), (0, 0), (0, 0)), mod4=3),
    "att_b8": _c("routenet", ATT, _ONE, G(3, 1, 1, seed=1), G(2, 2, 2, seed=2), cells=((1, 1, 1), (1, 1, 1), (2, 2)),
                 empty=((0, 0, 0), (0, 0, 0), (0, 0)), mod4=0),
    # group contents
    "att_hole": _c("routenet", ATT, _HOLE, G(3, 1, 1, seed=1), cells=((2, 0, 2), (1, 1, 1)),
                   empty=((0, 2, 0), (0, 0, 0)), mod4=2),   # group 1 has no cell, groups 0, 2 and 3 of its block do
    "att_dup": _c("routenet", ATT, _DUP, cells=((2, 2),), empty=((0, 0),), mod4=2, dup=True),   # summed LeakyReLUs
    "att_idle": _c("routenet", ATT, _IDLE, G(3, 1, 1, seed=1), cells=((3, 3, 3, 3), (1, 1, 1)),
                   empty=((1, 1, 1, 1), (0, 0, 0)), mod4=3),   # an idle link: mx starts at 0 in every group
    # attention, Q-size {link, node} -> path: late positions hold one path and P - 1 empties
    "qatt_p1": _c("qsize", ATT, G(1, 2, (2,), N=2), cells=((1, 1, 1, 1),), empty=((0, 0, 0, 0),), mod4=0),
    "qatt_p16": _qatt(16, 5),
    "qatt_p17": _qatt(17, 16),
    "qatt_p64": _qatt(64, 0),
    "qatt_p65": _qatt(65, 64),
    "qatt_mixed": _c("qsize", ATT, G(17, 4, tuple(1 + p % 3 for p in range(17)), N=5),
                     cells=((17, 17, 11, 11, 5, 5),), empty=((0, 0, 6, 6, 12, 12),), mod4=2),
    # logits: attention/attn_kernel scaled after init_params, on the 65-link graph (groups 1 and 2 hold empties)
    "logit_moderate": _c("routenet", ATT, _HOT65, scale=((ATTN_KERNEL, 60.0),), cells=((65, 2, 1),),
                         empty=((0, 63, 64),), mod4=3),   # the largest |e| lies in 5 .. 15
    # forward only: the softmax is one-hot to float precision, so its gradient carries no information.
    # e >= 90 and e <= -90: exp(e) alone overflows float32 and the empty cells' exp(-mx) is 0; the second
    # graph's groups of one cell and no empties score below -90 too, where exp(e - 0) is 0 and only e - mx is 1
    "logit_overflow": _c("routenet", ATT, _HOT65, G(3, 1, 1, seed=3), scale=((ATTN_KERNEL, 30000.0),), grads=False,
                         cells=((65, 2, 1), (1, 1, 1)), empty=((0, 63, 64), (0, 0, 0)), mod4=2),
    # convolution, RouteNet path -> link: deg = link 0's in-degree around the four-message unroll
    "conv_deg1": _c("routenet", CONV(), G(20, 4, _rand(20, 3, 30), hot=1), deg0=1),
    "conv_deg3": _c("routenet", CONV("tanh"), G(20, 4, _rand(20, 3, 31), hot=3), deg0=3),
    "conv_deg4": _c("routenet", CONV("selu"), G(20, 4, _rand(20, 3, 32), hot=4), deg0=4),
    "conv_deg5": _c("routenet", CONV(), G(20, 4, _rand(20, 3, 33), hot=5), deg0=5),
    "conv_deg64": _c("routenet", CONV(), G(80, 4, _rand(80, 3, 34), hot=64), deg0=64),
    # the link rows at the 16-row tile
    "conv_l15": _c("routenet", CONV("tanh"), G(40, 15, _rand(40, 3, 35))),
    "conv_l16": _c("routenet", CONV("selu"), G(40, 16, _rand(40, 3, 36))),
    "conv_l17": _c("routenet", CONV("relu"), G(40, 17, _rand(40, 3, 37))),
    # degree 0: the idle link's input is 0 / 0 as the reference divides; no path reads its state.  Autograd
    # carries the NaN into link_update/* and convolution/kernel alone; every other tensor is compared
    "conv_idle": _c("routenet", CONV("relu"), G(40, 15, _rand(40, 3, 38), idle_links=1), idle=15),
    "conv_idle_tanh": _c("routenet", CONV("tanh"), G(40, 15, _rand(40, 3, 38), idle_links=1), idle=15),
    "qconv_p17": _c("qsize", CONV("tanh"), _q(17, 16)),   # two sources: deg counts both
    # concat, Q-size, on slots (axis 1) and on features (axis 2)
    "cat1_p1": _c("qsize", CAT1, G(1, 2, (2,), N=2)),
    "cat1_p16": _c("qsize", CAT1, G(16, 4, _rand(16, 3, 40), N=4)),
    "cat1_p17": _c("qsize", CAT1, G(17, 4, _rand(17, 3, 41), N=4)),
    "cat1_len1": _c("qsize", CAT1, G(17, 4, 1, N=4)),   # one-step sequences: a link slot, then a node slot
    "cat1_long": _c("qsize", CAT1, _q(17, 8)),
    "cat2_p1": _c("qsize", CAT2, G(1, 2, (2,), N=2)),
    "cat2_p16": _c("qsize", CAT2, G(16, 4, _rand(16, 3, 40), N=4)),
    "cat2_p17": _c("qsize", CAT2, G(17, 4, _rand(17, 3, 41), N=4)),
    "cat2_len1": _c("qsize", CAT2, G(17, 4, 1, N=4)),   # one step of [link | node]
    "cat2_long": _c("qsize", CAT2, _q(17, 8)),
    # hidden size 16 (32 is every case above), and 64 where it is lowered: concat (REFUSED_H64 holds the rest)
    "att_h16": _c("routenet", ATT, _IDLE, _DUP, hidden=16, cells=((3, 3, 3, 3), (2, 2)), empty=((1, 1, 1, 1), (0, 0)),
                  mod4=2, dup=True),
    "qatt_h16": _c("qsize", ATT, _q(17, 16), hidden=16, cells=_qcells(17)[0], empty=_qcells(17)[1], mod4=2),
    "conv_h16": _c("routenet", CONV("selu"), G(20, 4, _rand(20, 3, 33), hot=5), hidden=16, deg0=5),
    "cat1_h16": _c("qsize", CAT1, G(17, 4, _rand(17, 3, 41), N=4), hidden=16),
    "cat2_h16": _c("qsize", CAT2, G(17, 4, _rand(17, 3, 41), N=4), hidden=16),
    "cat1_h64": _c("qsize", CAT1, G(17, 4, _rand(17, 3, 41), N=4), hidden=64),
    "cat2_h64": _c("qsize", CAT2, G(17, 4, _rand(17, 3, 41), N=4), hidden=64),   # two 64-wide slices of a 128-wide input
}
# attention and convolution are lowered for 16 and 32 units: plan creation refuses 64 with this status
# and text (both concat axes are lowered at 64)
REFUSED_H64 = {
    "att_h64": ("routenet", ATT, -2, "mp 1: attention / convolution lowered for 16 or 32 units"),
    "qatt_h64": ("qsize", ATT, -2, "mp 0: attention / convolution lowered for 16 or 32 units"),
    "conv_h64": ("routenet", CONV(), -2, "mp 1: attention / convolution lowered for 16 or 32 units"),
}

ATTENTION = sorted(n for n, c in CASES.items() if c.aggr == ATT)
CONVOLUTION = sorted(n for n, c in CASES.items() if c.aggr[0] == ("type", "convolution"))
CONCAT = sorted(n for n, c in CASES.items() if c.aggr[0] == ("type", "concat"))
BATCHES = sorted(n for n, c in CASES.items() if len(c.graphs) > 1)
DEG0 = sorted(n for n, c in CASES.items() if c.idle is not None)
GRADS = sorted(n for n, c in CASES.items() if c.grads and c.idle is None)


def model(kind, aggr, hidden):
    """(description, dims) of RouteNet / Q-size with the aggregation, T = 2, features taken as given."""
    if kind == "qsize":
        desc = model_examples.qsize_aggregation(dict(aggr), iterations=sc.ITERATIONS, hidden=hidden)
    else:
        desc = model_examples.routenet_aggregation(dict(aggr), hidden=hidden, iterations=sc.ITERATIONS)
    for e in desc["entities"]:
        for f in e["features"]:
            f["normalization"] = "None"
    return desc, sc.dims(kind)


def attention_tables(kind, g):
    """The attention MP's (destination, position) of every message of one graph and the destination count,
    from the arrays alone (the oracle's comb_dst / comb_seq, GM:528-541)."""
    if kind == "routenet":
        return np.asarray(g["dst_adj_paths_links"], np.int64), np.asarray(g["seq_path_link"], np.int64), int(g["num_link"])
    dl, dn = np.asarray(g["dst_adj_links_paths"], np.int64), np.asarray(g["dst_adj_nodes_paths"], np.int64)
    P = int(g["num_path"])
    pos_n = np.asarray(g["seq_node_path"], np.int64) + np.bincount(dn, minlength=P)[dn]
    return np.concatenate([dl, dn]), np.concatenate([np.asarray(g["seq_link_path"], np.int64), pos_n]), P


def groups(kind, g):
    """Per position of one graph: (cells, empty cells, the most messages in one cell)."""
    dst, pos, n = attention_tables(kind, g)
    out = []
    for q in range(int(pos.max()) + 1):
        _, counts = np.unique(dst[pos == q], return_counts=True)
        out.append((int(counts.size), n - int(counts.size), int(counts.max()) if counts.size else 0))
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(desc, dims, mi, plan, graphs, labels, parameters) of a table entry, built once per session."""
    c = CASES[name]
    desc, dims = model(c.kind, c.aggr, c.hidden)
    graphs = [sc.graph(g, c.kind) for g in c.graphs]
    mi = Model_information(copy.deepcopy(desc), dims)
    plan = MPPlan.from_model_info(mi)
    prm = plan.init_params(sc.SEED, bias_scale=sc.BIAS)
    for pname, factor in c.scale:
        prm[pname] = (np.asarray(prm[pname], np.float32) * np.float32(factor)).astype(np.float32)
    return desc, dims, mi, plan, graphs, sc.labels_for(graphs), prm


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.float64):
    """The oracle's (predictions, {entity: final states, graphs stacked}, attention scores per MP run) of a
    table entry, read-only."""
    from oracle.dense_forward import DenseOracle
    desc, dims, _, plan, graphs, _, prm = case_inputs(name)
    o = DenseOracle(desc, dims, prm, dtype=dtype)
    o.scores = []
    per = [o.final_states(g) for g in graphs]
    pred = np.concatenate([o._readout(s, g).reshape(-1) for s, g in zip(per, graphs)])
    states = {e: np.concatenate([s[e] for s in per], axis=0) for e in plan.entities}
    for a in [pred] + list(states.values()):
        a.setflags(write=False)
    return pred, states, o.scores


@functools.lru_cache(maxsize=None)
def grad_reference(name):
    """torch autograd of the float64 restatement on a table entry: (loss, l2, {name: gradient}, predictions)."""
    from oracle.train_oracle import TorchOracle
    desc, dims, _, _, graphs, labels, prm = case_inputs(name)
    return TorchOracle(desc, dims, prm).loss_and_grads(graphs, labels)
