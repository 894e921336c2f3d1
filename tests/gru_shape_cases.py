"""The option sets of tests/gru_cases.py on the graphs of tests/shape_cases.py: GRU cells with activation,
recurrent_activation, use_bias and reset_after at the row-tile, step, in-degree and block edges of
gru_cell.hip's four kernels, which copy the default kernels' structure by hand, and on the pre-summed
route of mp_step.cpp (a plan with any option cell sends rows of >= 64 messages through launch_sum_seg /
launch_sum_win and an identity CSR, in the training forward too).  Shared by tests/test_gru_shape_cases.py
(CPU) and tests/test_gpu_gru_shapes.py.

CASES is {name: (shape, options, model kwargs)}: ``shape`` a shape_cases.Shape (graphs, hidden, kind, env),
``options`` the GRUCell keys, ``model kwargs`` gru_cases._routenet's ``widths`` / ``aggregation`` (Q-size
entries give the options to the path cell alone, gru_cases._qsize_path).  Names are "<shape>/<option set>"
with "/<model>" after it where the model is not plain RouteNet / Q-size.  KIND names the kind of edge each
entry is there for.  T = 2, normalization "None", seeds and labels as shape_cases (sc.inputs_for).

Every shape takes V1 (reset_after false: the second K = H sweep, gu2 / rh scratch, dU from two
contractions); ALL_FOUR, HS + NO_BIAS and RELU are met once at each kind of edge.  RELU is not put on p257:
about 128 messages per link into an unbounded candidate take the states to 70 there, and 4 x the float32
run's error (9.3e-5) leaves no room below TOL.

Which kernels beyond gru_cases' own list an entry reaches:

  h64_l191 / l192 / l193   sum_gru_cell<64,64>'s LDS form: 12 waves x 16 rows = 192 rows per block of a
                           persistent grid; 193 rows leave a second block one row in its wave 0
  deg64 deg65 *_win h*_deg64 qs_node64   the pre-summed route (x_save written by the identity-CSR step)
  qs_*                     two cell kinds in one plan: the default link / node cells' sums move onto the
                           pre-summed route with the path cell's options
No GPU is needed here."""
import functools

import numpy as np

from tests import gru_cases as gc
from tests import shape_cases as sc

T = sc.ITERATIONS
OPTIONS = {"V1": gc.V1, "ALL_FOUR": gc.ALL_FOUR, "HS_NO_BIAS": dict(gc.HS, **gc.NO_BIAS), "RELU": gc.RELU}

# the H = 64 LDS form's 192-row block: paths of length 2, so 200 messages cross 191 .. 193 links
H64_ROWS = {"h64_l%d" % L: sc._s(sc.G(100, L, 2), hidden=64) for L in (191, 192, 193)}

ORDERED = ["p1", "p16", "p17", "p33", "p63", "p64", "p65", "p129", "p257", "b16_16", "b_p1_between"]
LENGTHS = ["len_all_1", "len_all_L", "long16_first", "long16_mid", "long16_last", "long17_mid", "long33_first",
           "long33_mid", "long33_last"]
SUM_ROWS = ["l1", "l16", "l17", "l33", "l15_idle", "l16_idle"]
DEGREES = ["deg0", "deg1", "deg63", "deg64", "deg65", "deg64_win", "deg65_win"]
WIDTHS = ["h16_p17", "h16_deg64", "h64_p17", "h64_deg64"]
QSIZE = ["qs_n1", "qs_n17", "qs_node64"]
L16_P32 = {"widths": {"link": 16, "path": 32}}
AGGREGATIONS = {"attention": {"aggregation": {"type": "attention"}}, "convolution": {"aggregation": {"type": "convolution"}}}

CASES, KIND = {}, {}


def _add(kind, shape, option, tag=None, **kw):
    name = "/".join([shape, option] + ([tag] if tag else []))
    assert name not in CASES
    CASES[name] = (H64_ROWS[shape] if shape in H64_ROWS else sc.SHAPES[shape], OPTIONS[option], kw)
    KIND[name] = kind


for _kind, _shapes in (("ordered_rows", ORDERED), ("path_lengths", LENGTHS), ("sum_rows", SUM_ROWS),
                       ("in_degree", DEGREES), ("other_widths", WIDTHS), ("lds_block", sorted(H64_ROWS)),
                       ("qsize", QSIZE)):
    for _shape in _shapes:
        _add(_kind, _shape, "V1")
for _shape in ("l17", "deg64"):
    _add("other_widths", _shape, "V1", "l16_p32", **L16_P32)
for _tag, _kw in sorted(AGGREGATIONS.items()):   # (no idle link under convolution: 0 / 0, aggregation_cases' case)
    for _shape in ("l17", "deg1", "deg65"):
        _add(_tag, _shape, "V1", _tag, **_kw)
# the other option sets, once at each kind of edge
for _kind, _all_four, _hs_no_bias, _relu in (("ordered_rows", "p257", "p65", "p17"),
                                             ("path_lengths", "long33_mid", "long16_first", "long17_mid"),
                                             ("sum_rows", "l17", "l16_idle", "l15_idle"),
                                             ("in_degree", "deg65", "deg64_win", "deg64"),
                                             ("other_widths", "h64_deg64", "h16_p17", "h64_p17")):
    _add(_kind, _all_four, "ALL_FOUR")
    _add(_kind, _hs_no_bias, "HS_NO_BIAS")
    _add(_kind, _relu, "RELU")
SPREAD_KINDS = ("ordered_rows", "path_lengths", "sum_rows", "in_degree", "other_widths")

TS_CASES = ["p33/V1", "p129/V1", "long33_mid/V1", "qs_n17/V1"]      # one child process under IGN_TS_MIN_ROWS=32
ADAM_CASES = ["deg65/ALL_FOUR", "h64_l193/V1"]
FEATURE_GRAD_CASES = ["p17/V1", "deg64/V1"]


def max_in_degree(name):
    """The largest number of messages into one link or node row of an entry's graphs: from 64 on
    (kSegMinMessages), or under IGN_SUM_WINDOW=1, a plain sum MP takes the pre-summed route."""
    graphs = case_inputs(name)[4]
    keys = ["dst_adj_paths_links"] + (["dst_adj_paths_nodes"] if CASES[name][0].kind == "qsize" else [])
    return max(int(np.bincount(np.asarray(g[k], np.int64)).max()) for g in graphs for k in keys)


def model(name):
    """(description, dims) of an entry: gru_cases' builders' descriptions (their NSFNET samples are not
    used), features taken as given."""
    s, options, kw = CASES[name]
    if s.kind == "qsize":
        assert not kw and s.hidden == 32
        desc = gc._qsize_path(options)()[0]
    else:
        desc = gc._routenet(options, hidden=s.hidden, **kw)()[0]
    assert desc["message_passing"]["num_iterations"] == T
    for e in desc["entities"]:
        for f in e["features"]:
            f["normalization"] = "None"
    return desc, sc.dims(s.kind)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(desc, dims, mi, plan, graphs, labels, parameters) of an entry, built once per session."""
    s = CASES[name][0]
    desc, dims = model(name)
    graphs = [sc.graph(g, s.kind) for g in s.graphs]
    mi, plan, labels, prm = sc.inputs_for(desc, dims, graphs)
    return desc, dims, mi, plan, graphs, labels, prm


def _reference(name, dtype):
    desc, dims, _, plan, graphs, _, prm = case_inputs(name)
    ora = gc.CellDenseOracle(desc, dims, prm, dtype=dtype)
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
    """gru_cases.float32_error's definition on an entry: the maximum scaled error (|a - b| / max(1, |b|))
    of a float32 numpy run of the restatement against its float64 run, over the predictions and every
    entity's final states."""
    p32, s32 = _reference(name, np.float32)
    p64, s64 = reference(name)
    err = lambda a, b: float((np.abs(np.asarray(a, np.float64) - b) / np.maximum(1.0, np.abs(b))).max())
    return max([err(p32, p64)] + [err(s32[e], s64[e]) for e in s64])


@functools.lru_cache(maxsize=None)
def autograd(name):
    """CellTorchOracle.loss_and_grads of an entry: (loss, l2 term, {tensor: gradient}, predictions)."""
    desc, dims, _, _, graphs, labels, prm = case_inputs(name)
    return gc.CellTorchOracle(desc, dims, prm).loss_and_grads(graphs, labels)
