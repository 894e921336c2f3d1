"""Graphs built at the routing level, so that a test chooses the row counts the kernels tile over: P paths
(the ordered update's, the readout's and the loss's rows), L links (the sum update's rows), each path's
length and a link's in-degree.  All-pairs shortest-path topologies (synthetic.routenet_sample) give every
link a path, bound every path by the diameter and never land a row count on a multiple of 16.

routenet_arrays / qsize_arrays return the generator's feature-dict contract directly;
routenet_sample_of / qsize_sample_of restate a built graph as the dataset sample whose generator output it
is (tests/test_shape_cases.py runs that through generator.sample_to_data and compares).

SHAPES is the table tests/test_gpu_shapes.py sweeps: H = 32 and T = 2 unless an entry says otherwise,
init_params(SEED, bias_scale=BIAS), at most 257 paths and 35 links per graph.  No GPU is needed here."""
import collections
import copy
import functools

import numpy as np

from ignnition_amd import model_examples, workloads
from ignnition_amd.engine import MPPlan
from ignnition_amd.json_operations import Model_information

SEED, BIAS, ITERATIONS = 5, 0.1, 2


def _route(P, n, lens, rng, hot):
    """Per path, lens[p] distinct rows of 0 .. n - 1 in a shuffled order: consecutive rows of one cursor
    that wraps, so every row is taken once sum(lens) >= n.  hot=k: row 0 leaves that pool and is added to
    exactly k paths (every path of length n among them)."""
    lens = np.asarray(lens, np.int64)
    assert lens.shape == (P,) and lens.min() >= 1 and lens.max() <= n
    pool = np.arange(n) if hot is None else np.arange(1, n)
    chosen = np.zeros(P, bool)
    if hot is not None:
        full = np.flatnonzero(lens == n)
        assert full.size <= hot <= P, "hot=%d cannot hold the %d paths that cross every row" % (hot, full.size)
        rest = np.setdiff1d(np.arange(P), full)
        chosen[full] = True
        chosen[rng.choice(rest, hot - full.size, replace=False)] = True
    routes, c = [], 0
    for p in range(P):
        k = int(lens[p]) - int(chosen[p])
        r = pool[(c + np.arange(k)) % max(pool.size, 1)] if k else np.zeros(0, np.int64)
        c += k
        routes.append(rng.permutation(np.concatenate([r, [0]]) if chosen[p] else r).astype(np.int64))
    return routes


def _adjacency(routes, P, n_rows, src):
    """The two index triples of one routing: rows -> paths in path order with positions 0 .. len - 1, and
    paths -> rows grouped per row in path order (the recipe of test_resident_falls_back_beyond_16bit_rows)."""
    lens = np.array([r.size for r in routes])
    dst_rp = np.repeat(np.arange(P), lens)
    rows = np.concatenate(routes)
    order = np.argsort(rows, kind="stable")   # per row, its messages in path order
    deg = np.bincount(rows, minlength=n_rows)
    return {"src_adj_%ss_paths" % src: list(rows), "dst_adj_%ss_paths" % src: list(dst_rp),
            "seq_%s_path" % src: list(np.concatenate([np.arange(k) for k in lens])),
            "src_adj_paths_%ss" % src: list(dst_rp[order]), "dst_adj_paths_%ss" % src: list(rows[order]),
            "seq_path_%s" % src: list(np.concatenate([np.arange(c) for c in deg]).astype(np.int64))}, deg


def _check_degrees(deg, n, idle, hot, lens):
    assert deg.size == n + idle and np.all(deg[n:] == 0), "an idle row is crossed"
    assert deg.sum() == int(np.sum(lens))
    if hot is not None:
        assert deg[0] == hot, "row 0 is crossed by %d paths, not %d" % (deg[0], hot)
    assert np.all(deg[1 if hot is not None else 0:n] >= 1), "a row that is not idle is crossed by no path"


def routenet_arrays(P, L, lens, seed, idle_links=0, hot=None, link_positions=()):
    """One RouteNet input dict: P paths over L crossed links (+ idle_links that no path crosses), path p
    over lens[p] distinct links at positions 0 .. lens[p] - 1 (no holes, so sequence_mask(final_len) is as
    wide as the padding); hot=k: link 0 is crossed by exactly k paths.  Features uniform in [-1, 1).
    link_positions: (link, positions) pairs that replace the seq_path_link values 0 .. deg - 1 of that
    link's messages (in path order): a repeated value puts two messages into one (link, position) cell,
    a skipped one leaves a position that this link does not fill."""
    rng = np.random.default_rng(seed)
    routes = _route(P, L, lens, rng, hot)
    g, deg = _adjacency(routes, P, L + idle_links, "link")
    _check_degrees(deg, L, idle_links, hot, lens)
    for link, positions in link_positions:
        at = np.flatnonzero(np.asarray(g["dst_adj_paths_links"]) == link)
        assert at.size == len(positions), "link %d has %d messages, not %d" % (link, at.size, len(positions))
        for k, q in zip(at, positions):
            g["seq_path_link"][k] = np.int64(q)
    assert max(g["seq_link_path"]) + 1 == int(np.max(lens))
    assert np.array_equal(np.bincount(g["dst_adj_links_paths"], minlength=P), np.asarray(lens))
    g.update(link_capacity=rng.uniform(-1, 1, L + idle_links).astype(np.float32),
             traffic=rng.uniform(-1, 1, P).astype(np.float32), num_link=L + idle_links, num_path=P)
    return g


def qsize_arrays(P, L, N, lens, seed, hot_node=None):
    """The Q-size counterpart: the same link routing, and path p over lens[p] distinct nodes of N (one per
    link it crosses); the interleave pattern is [node, link], so the padded sequence has 2 max(lens) slots,
    nodes on the even ones.  hot_node=k: node 0 receives exactly k messages."""
    g = routenet_arrays(P, L, lens, seed)
    rng = np.random.default_rng(seed + 1000)
    nodes, deg = _adjacency(_route(P, N, lens, rng, hot_node), P, N, "node")
    _check_degrees(deg, N, 0, hot_node, lens)
    m = int(np.max(lens))
    g.update(nodes, queue_sizes=rng.uniform(-1, 1, N).astype(np.float32), num_node=N,
             indices_node_to_path=list(range(0, 2 * m, 2)), indices_link_to_path=list(range(1, 2 * m, 2)))
    return g


def _sample_of(g, kinds):
    """The dataset sample (entities in link, path, node order; adjacencies keyed by destination, in
    destination order, destinations without a message absent) whose generator output is ``g``."""
    P = int(g["num_path"])
    s = {"entities": {}, "traffic": [float(x) for x in g["traffic"]], "delay": [1.0] * P}
    for k, feat in kinds:
        for i in range(int(g["num_" + k])):
            s["entities"]["%s%d" % (k[0], i)] = k
        s[feat] = [float(x) for x in g[feat]]
        if k == "link":
            for i in range(P):
                s["entities"]["p%d" % i] = "path"
    for k, _ in kinds:
        to_path, to_row = {}, {}
        for r, p in zip(g["src_adj_%ss_paths" % k], g["dst_adj_%ss_paths" % k]):
            to_path.setdefault("p%d" % p, []).append("%s%d" % (k[0], r))
        for p, r in zip(g["src_adj_paths_%ss" % k], g["dst_adj_paths_%ss" % k]):
            to_row.setdefault("%s%d" % (k[0], r), []).append("p%d" % p)
        s["adj_%ss_paths" % k], s["adj_paths_%ss" % k] = to_path, to_row
    return s


def routenet_sample_of(g):
    return _sample_of(g, [("link", "link_capacity")])


def qsize_sample_of(g):
    return dict(_sample_of(g, [("link", "link_capacity"), ("node", "queue_sizes")]), path_interleave=["node", "link"])


# ---------------------------------------------------------------------------------------------
# the table
def _rand(P, hi, seed=0):
    """P path lengths uniform in 1 .. hi."""
    return tuple(int(x) for x in np.random.default_rng(100 + seed).integers(1, hi + 1, P))


def _one_long(P, long, at):
    """Length ``long`` for path ``at``, 1 for every other."""
    return tuple(long if p == at else 1 for p in range(P))


def G(P, L, lens, seed=0, **kw):
    """One graph's routenet_arrays / qsize_arrays arguments (lens: one length for every path, or P lengths)."""
    return (("P", P), ("L", L), ("lens", (lens,) * P if isinstance(lens, int) else tuple(lens)), ("seed", seed)) + \
        tuple(sorted(kw.items()))


Shape = collections.namedtuple("Shape", "graphs hidden kind env")


def _s(*graphs, hidden=32, kind="routenet", env=()):
    return Shape(tuple(graphs), hidden, kind, tuple(env))


_WIN = (("IGN_SUM_WINDOW", "1"),)
SHAPES = {
    # P: the rows of the ordered update, the readout and the loss
    "p1": _s(G(1, 3, (3,))),                    # one row: every 16-row tile, 64-row grid and 256-thread block mostly empty
    "p15": _s(G(15, 5, _rand(15, 4))),          # one short 16-row tile
    "p16": _s(G(16, 5, _rand(16, 4))),          # exactly one full tile: the row mask's last lane
    "p17": _s(G(17, 5, _rand(17, 4))),          # a full tile and a one-row tile: a wave's second tile
    "p31": _s(G(31, 5, _rand(31, 4))),          # two tiles of one wave, the second short
    "p32": _s(G(32, 5, _rand(32, 4))),          # two full tiles: one wave's pair exactly
    "p33": _s(G(33, 5, _rand(33, 4))),          # a second wave of one row; with IGN_TS_MIN_ROWS=32 a second chunk of one row
    "p63": _s(G(63, 5, _rand(63, 4))),          # one row short of the (n + 63) / 64 grids' block
    "p64": _s(G(64, 5, _rand(64, 4))),          # exactly one 64-row block
    "p65": _s(G(65, 5, _rand(65, 4))),          # a second 64-row block of one row
    "p127": _s(G(127, 5, _rand(127, 4))),       # one row short of the readout's 128-row group and ts_plan's chunk floor
    "p128": _s(G(128, 5, _rand(128, 4))),       # exactly one 128-row group / one full chunk
    "p129": _s(G(129, 5, _rand(129, 4))),       # a second group of one row; ts_plan: two chunks, 80 + 49 rows
    "p257": _s(G(257, 5, _rand(257, 4))),       # the 256-thread loss block and one row; three 128-row groups
    # L: the rows of the sum update
    "l1": _s(G(20, 1, 1)),                      # one link row, every path crossing it
    "l2": _s(G(20, 2, _rand(20, 2, 1))),        # two rows of one tile
    "l15": _s(G(40, 15, _rand(40, 3, 2))),      # one short tile
    "l16": _s(G(40, 16, _rand(40, 3, 3))),      # one full tile: the header prefetch's min(tile, n_tiles - 1) at its edge
    "l17": _s(G(40, 17, _rand(40, 3, 4))),      # a full tile and a one-row tile
    "l33": _s(G(40, 33, _rand(40, 3, 5))),      # three tiles, the last of one row: a wave's second tile and a second wave
    "l15_idle": _s(G(40, 15, _rand(40, 3, 6), idle_links=1)),   # 16 rows, the idle link in the tile's last slot
    "l16_idle": _s(G(40, 16, _rand(40, 3, 7), idle_links=1)),   # 17 rows, the idle link alone in the last tile
    # in-degree of link 0: the lane walk / segmented sum switch (kSegMinMessages = 64)
    "deg0": _s(G(80, 4, _rand(80, 3, 8), hot=0)),      # link 0 idle in the first slot
    "deg1": _s(G(80, 4, _rand(80, 3, 9), hot=1)),      # one message: the lane walk's shortest chain
    "deg63": _s(G(80, 4, _rand(80, 3, 10), hot=63)),   # the longest lane walk
    "deg64": _s(G(80, 4, _rand(80, 3, 11), hot=64)),   # the first segmented row
    "deg65": _s(G(80, 4, _rand(80, 3, 12), hot=65)),   # a segmented row with a message past the wave's 64 lanes
    "deg64_win": _s(G(80, 4, _rand(80, 3, 11), hot=64), env=_WIN),   # the windowed sum at the same edge (not resident)
    "deg65_win": _s(G(80, 4, _rand(80, 3, 12), hot=65), env=_WIN),
    # path lengths
    "len_all_1": _s(G(24, 7, 1)),               # every row of every tile has length 1: one step, no tail
    "len_all_L": _s(G(10, 6, 6)),               # every path crosses every link: no row leaves a tile early
    "long2_first": _s(G(20, 2, _one_long(20, 2, 0))),      # one long row among length-1 rows: the tile's steps are
    "long2_mid": _s(G(20, 2, _one_long(20, 2, 8))),        # its longest row's, every other row masked after step 0;
    "long2_last": _s(G(20, 2, _one_long(20, 2, 19))),      # first / middle / last in path order (the length sort
    "long16_first": _s(G(20, 16, _one_long(20, 16, 0))),   # moves it to the tile's first row: the header order)
    "long16_mid": _s(G(20, 16, _one_long(20, 16, 8))),     # L = 16: the long row's codes fill one 16-step group
    "long16_last": _s(G(20, 16, _one_long(20, 16, 19))),
    "long17_first": _s(G(20, 17, _one_long(20, 17, 0))),   # L = 17: one step past it
    "long17_mid": _s(G(20, 17, _one_long(20, 17, 8))),
    "long17_last": _s(G(20, 17, _one_long(20, 17, 19))),
    "long33_first": _s(G(20, 33, _one_long(20, 33, 0))),   # L = 33: three link tiles, a sequence of 33 steps
    "long33_mid": _s(G(20, 33, _one_long(20, 33, 8))),
    "long33_last": _s(G(20, 33, _one_long(20, 33, 19))),
    # batches whose row counts add up to a tile edge
    "b15_1": _s(G(15, 15, _rand(15, 3, 13)), G(1, 1, 1)),   # 16 rows over two graphs: the last row is a graph
    "b16_16": _s(G(16, 16, _rand(16, 3, 14)), G(16, 16, _rand(16, 3, 15), seed=1)),   # a graph boundary on the tile edge
    "b17_15_32": _s(G(17, 17, _rand(17, 3, 16)), G(15, 15, _rand(15, 3, 17), seed=1),
                    G(32, 32, _rand(32, 3, 18), seed=2)),   # a boundary inside a tile, then on a 32-row and a 64-row edge
    "b_p1_between": _s(G(20, 5, _rand(20, 4, 19)), G(1, 1, 1, seed=1), G(33, 6, _rand(33, 4, 20), seed=2)),   # a one-row graph inside
    # the other hidden sizes (no resident forward: the batched kernels at DIN = H = 16 / 64)
    "h16_p1": _s(G(1, 3, (3,)), hidden=16),
    "h16_p16": _s(G(16, 5, _rand(16, 4)), hidden=16),
    "h16_p17": _s(G(17, 5, _rand(17, 4)), hidden=16),
    "h16_deg64": _s(G(80, 4, _rand(80, 3, 11), hot=64), hidden=16),
    "h64_p1": _s(G(1, 3, (3,)), hidden=64),
    "h64_p16": _s(G(16, 5, _rand(16, 4)), hidden=64),
    "h64_p17": _s(G(17, 5, _rand(17, 4)), hidden=64),
    "h64_deg64": _s(G(80, 4, _rand(80, 3, 11), hot=64), hidden=64),
    # Q-size: the node rows of the second sum update and the union-row tiles of links + nodes
    "qs_n1": _s(G(6, 3, 1, N=1), kind="qsize"),                     # one node row, one slot pair
    "qs_n16": _s(G(20, 6, _rand(20, 4, 21), N=16), kind="qsize"),   # one full node tile
    "qs_n17": _s(G(20, 6, _rand(20, 4, 22), N=17), kind="qsize"),   # a node tile of one row
    "qs_node64": _s(G(80, 5, _rand(80, 3, 23), N=4, hot_node=64), kind="qsize"),   # a node's first segmented sum
}
# the P sweep's graphs, for the tests that put another model on them (Dense stacks, Dropout, the losses)
P_GRAPH = {p: SHAPES["p%d" % p].graphs[0] for p in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)}


@functools.lru_cache(maxsize=None)
def graph(spec, kind="routenet"):
    """The input dict of one G(...) (built once; callers do not modify it)."""
    return (qsize_arrays if kind == "qsize" else routenet_arrays)(**dict(spec))


def model(kind, hidden, iterations=ITERATIONS):
    """(description, dims) of RouteNet / Q-size at one hidden size, features taken as given (no
    normalization: the builders draw them in [-1, 1))."""
    desc = (model_examples.qsize if kind == "qsize" else model_examples.routenet)(hidden=hidden, iterations=iterations)
    for e in desc["entities"]:
        for f in e["features"]:
            f["normalization"] = "None"
    return desc, dims(kind)


@functools.lru_cache(maxsize=None)
def dims(kind):
    """The feature / adjacency dimensions of the example datasets."""
    return workloads.model(kind)[1]


def labels_for(graphs, units=1, seed=7):
    """Labels uniform in [1, 2): away from the predictions, which these parameters keep within (-1, 1), so
    that the squared-error loss is well conditioned even over one row (well_conditioned)."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(1.0, 2.0, (int(g["num_path"]), units)).astype(np.float32).reshape(-1) for g in graphs]


def well_conditioned(labels, pred):
    """The mean squared error's relative condition number against a perturbation delta of the predictions
    is at most 2 delta / rms(y - p): with rms >= 0.25 and float32 predictions below 1 (delta <= 6e-8 per
    rounding), a loss compared at 1e-5 relative has a margin of 20 roundings.  A single label that lands
    within 5e-3 of its prediction (P = 1, normal labels) has none: one ulp of the prediction moves the loss
    by 2.6e-5."""
    d = np.concatenate([np.asarray(l, np.float64).reshape(-1) for l in labels]) - np.asarray(pred, np.float64).reshape(-1)
    assert np.abs(np.asarray(pred)).max() < 1.0 and np.sqrt(np.mean(d * d)) >= 0.25


def inputs_for(desc, dims, graphs, units=1):
    """(mi, plan, labels, parameters) of a description on built graphs."""
    mi = Model_information(copy.deepcopy(desc), dims)
    plan = MPPlan.from_model_info(mi)
    return mi, plan, labels_for(graphs, units), plan.init_params(SEED, bias_scale=BIAS)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(desc, dims, mi, plan, graphs, labels, parameters) of a table entry, built once per session."""
    s = SHAPES[name]
    desc, dims = model(s.kind, s.hidden)
    graphs = [graph(g, s.kind) for g in s.graphs]
    mi, plan, labels, prm = inputs_for(desc, dims, graphs)
    return desc, dims, mi, plan, graphs, labels, prm


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle's predictions of a table entry, read-only."""
    from oracle.dense_forward import DenseOracle
    desc, dims, _, _, graphs, _, prm = case_inputs(name)
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def grad_reference(name):
    """torch autograd of the float64 restatement on a table entry: (loss, l2, {name: gradient}, predictions)."""
    from oracle.train_oracle import TorchOracle
    desc, dims, _, _, graphs, labels, prm = case_inputs(name)
    o = TorchOracle(desc, dims, prm).loss_and_grads(graphs, labels)
    well_conditioned(labels, o[3])
    return o
