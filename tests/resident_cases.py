"""Graphs that sit on the graph-resident forward's dynamic-LDS budget and on the switches between its
forms (ignnition_amd/csrc/resident.hip; decided on the host by lower_resident in batch_lower.cpp and
resident_batch in engine.cpp), and the byte formula restated from the kernel's own carve-up of that LDS.

One workgroup runs a group of K consecutive graphs as one disjoint union.  With U union rows (links, then
nodes), M messages of the sum MPs, P path rows and C = sum(sequence lengths) + longest + 8 step codes, the
kernel lays out, in this order, from the start of its dynamic LDS:

    all-LDS form only     float  path states   [P][SP]
    every form            float  union states  [U][SP]
                          float  table         [U + 1][ST]      (the hole row last)
                          int32  CSR pointers  [U + 1]
                          uint16 row order     [(U + 1) & ~1]   (padded to an even count)
    not CSR-global        uint16 message rows  [M]
    all-LDS form only     uint16 step codes    [C]

Form 0 (all-LDS) where the largest group's bytes fit LIMIT, else form 1 (path states and codes in global
memory) where that fits, else form 2 (the message rows too), else the batched launches.  With no
IGN_RES_GROUP, two graphs share a workgroup where the single-graph all-LDS bytes fit twice.

CASES is the table tests/test_gpu_resident_cases.py runs; every entry's expected resident_info fields come
from ``expected`` here, never from the engine.  Graphs are shape_cases' (H = 32, T = 2, SEED / BIAS,
labels_for).  No GPU is needed here."""
import collections
import functools

import numpy as np

from tests import shape_cases as sc
from tests.shape_cases import G

LIMIT = 144 * 1024           # kResidentMaxDynLds
SP, ST = 36, 100             # floats per LDS state row / projected-table row
MAX_TILES = 32               # kResidentMaxTiles: union-row tiles of one workgroup (links' + nodes')
MAX_ROWS = 65535             # local rows are 16-bit


# ---------------------------------------------------------------------------------------------
# the restatement
Counts = collections.namedtuple("Counts", "U M P C tiles")


def counts(graphs, kind):
    """U, M, P, C and the union-row tiles of one workgroup's group of built graphs."""
    ents = ("link", "node") if kind == "qsize" else ("link",)
    rows = [sum(int(g["num_" + e]) for g in graphs) for e in ents]
    M = sum(len(g["src_adj_paths_%ss" % e]) for g in graphs for e in ents)
    seq = np.concatenate([np.bincount(np.asarray(g["dst_adj_links_paths"]), minlength=int(g["num_path"])) for g in graphs])
    seq = seq * len(ents)    # Q-size interleaves a node and a link per hop
    return Counts(sum(rows), M, int(seq.size), int(seq.sum() + seq.max() + 8), sum((r + 15) // 16 for r in rows))


def lds_bytes(c, form):
    b = 4 * (c.U * SP + (c.U + 1) * ST) + 4 * (c.U + 1) + 2 * ((c.U + 1) & ~1)
    if form != 2:
        b += 2 * c.M
    if form == 0:
        b += 4 * c.P * SP + 2 * c.C
    return b


def _lower(graphs, kind, K, force_pg):
    """lower_resident at K graphs per workgroup: None where the batch does not lower."""
    groups = [counts(graphs[i:i + K], kind) for i in range(0, len(graphs), K)]
    if any(c.P > MAX_ROWS or c.U > MAX_ROWS or c.tiles > MAX_TILES for c in groups):
        return None
    lds = [max(lds_bytes(c, f) for c in groups) for f in range(3)]
    form = 0
    if lds[0] > LIMIT or force_pg:
        form = 1 if lds[1] <= LIMIT else 2
        if lds[form] > LIMIT:
            return None
    return {"active": 1, "form": form, "lds_bytes": lds[form], "graphs_per_workgroup": K, "workgroups": len(groups),
            "train_form": 1 if lds[1] <= LIMIT else 2, "lds": lds}


def expected(graphs, kind, group=0, force_pg=False):
    """The resident_info fields of a batch (plus train_form and the three forms' bytes): group is
    IGN_RES_GROUP (0: the automatic rule), force_pg is IGN_RESIDENT=2."""
    one = _lower(graphs, kind, group or 1, force_pg)
    if one is None:
        return {"active": 0}
    if group == 0 and one["form"] == 0 and len(graphs) >= 2 and 2 * one["lds"][0] <= LIMIT:
        two = _lower(graphs, kind, 2, force_pg)
        if two is not None:
            return two
    return one


FIELDS = ("active", "form", "lds_bytes", "graphs_per_workgroup", "workgroups")


# ---------------------------------------------------------------------------------------------
# the table
def _lens(P, hi, total, seed):
    """P path lengths in 1 .. hi that add up to total: shape_cases' draw, then single lengths moved by one."""
    lens = list(sc._rand(P, hi, seed))
    assert P <= total <= P * hi
    i = 0
    while sum(lens) != total:
        d = 1 if sum(lens) < total else -1
        if 1 <= lens[i % P] + d <= hi:
            lens[i % P] += d
        i += 1
    return tuple(lens)


def _mix(*runs):
    """(count, length) runs, e.g. (891, 4), (11, 3)."""
    return tuple(k for n, k in runs for _ in range(n))


Case = collections.namedtuple("Case", "graphs kind group edge side grads poison")


def _c(*graphs, kind="routenet", group=0, edge=None, side=None, grads=False, poison=False):
    return Case(tuple(graphs), kind, group, edge, side, grads, poison)


_TINY = G(3, 2, (1, 2, 1), seed=9)
_A_FIT = G(902, 5, _mix((891, 4), (11, 3)))            # M = 3597, C = 3609: 3156 + 7194 + 129 888 + 7218 = 147 456
_A_OVER = G(902, 5, _mix((892, 4), (10, 3)))           # one length-3 path lengthened: one message and one code more
_D_FIT = [G(441, 5, _mix((438, 4), (3, 3)), seed=s) for s in range(3)]    # M = 1761: 73 728, half the budget
_D_OVER = [G(441, 5, _mix((439, 4), (2, 3)), seed=s) for s in range(2)]   # 73 732
_B = lambda total, seed=0, **kw: G(700, 260, _lens(700, 4, total, seed), seed=seed, **kw)   # 143 404 + 2 M
_Q = dict(kind="qsize")
_E_A_FIT = G(767, 13, _mix((758, 4), (9, 3)), N=9)              # U = 22: 12 504 + 8 * 3059 + 144 * 767 + 32
_E_A_OVER = G(767, 13, _mix((1, 5), (756, 4), (10, 3)), N=9)    # the same messages, the longest path one hop longer
_E_B = lambda total: G(400, 200, _lens(400, 4, total, 40), N=60)   # U = 260 as B, M = 2 * total; nodes from row 200

CASES = {
    # A. all-LDS <-> path-global
    "a_fit": _c(_A_FIT, edge="A", side="fit", grads=True, poison=True),
    "a_over": _c(_A_OVER, edge="A", side="over", grads=True),
    "a_fit_after_tiny": _c(_TINY, _A_FIT, edge="A", side="fit", grads=True, poison=True),   # the form is the maximum over
    "a_over_after_tiny": _c(_TINY, _A_OVER, edge="A", side="over", grads=True),             # graphs: the tiny one runs it too
    # B. path-global <-> CSR-global
    "b_fit": _c(_B(2026), edge="B", side="fit", grads=True, poison=True),
    "b_over": _c(_B(2027), edge="B", side="over", grads=True),
    "b_over_hot63": _c(_B(2027, 1, hot=63), edge="B", side="over"),   # the lane walk / segmented sum switch with the
    "b_over_hot64": _c(_B(2027, 2, hot=64), edge="B", side="over"),   # message rows read from L2 (!CL)
    "b_over_hot65": _c(_B(2027, 3, hot=65), edge="B", side="over"),
    "b_idle_last": _c(G(800, 255, _lens(800, 5, 3127, 4), seed=4, idle_links=1), edge="B", side="over"),   # U = 256: 141 204 + 2 M
    # C. CSR-global <-> the batched launches
    "c_fit": _c(G(300, 267, _lens(300, 4, 700, 5), seed=5), edge="C", side="fit"),      # 147 256
    "c_fallback": _c(G(300, 268, _lens(300, 4, 700, 6), seed=6), edge="C", side="over"),   # 147 804
    # D. two graphs per workgroup
    "d_fit2": _c(*_D_FIT[:2], edge="D", side="fit", grads=True, poison=True),
    "d_over2": _c(*_D_OVER, edge="D", side="over", grads=True),
    "d_fit3": _c(*_D_FIT, edge="D", side="fit", grads=True, poison=True),           # the last group is short
    "d_group_pg": _c(G(550, 74, _lens(550, 4, 1400, 7), seed=7), G(552, 74, _lens(552, 4, 1390, 8), seed=8), group=2),
    "d_group_268": _c(G(200, 134, _lens(200, 3, 400, 9), seed=9), G(200, 134, _lens(200, 3, 410, 10), seed=10), group=2),
    # E. Q-size: links and nodes split unevenly, the nodes' union rows start inside a tile
    "e_a_fit": _c(_E_A_FIT, edge="A", side="fit", **_Q),
    "e_a_over": _c(_E_A_OVER, edge="A", side="over", **_Q),
    "e_b_fit": _c(_E_B(1013), edge="B", side="fit", grads=True, **_Q),
    "e_b_over": _c(_E_B(1014), edge="B", side="over", grads=True, **_Q),
}
# the 16-bit local rows under IGN_RES_GROUP=2: 65 535 path rows in one group, and one more
ROWS16 = {
    "d_16bit_fit": _c(G(32768, 8, sc._rand(32768, 3, 30)), G(32767, 8, sc._rand(32767, 3, 31), seed=1), group=2),
    "d_16bit_over": _c(G(32768, 8, sc._rand(32768, 3, 30)), G(32768, 8, sc._rand(32768, 3, 32), seed=1), group=2),
}
EXACT = {"A": LIMIT, "B": LIMIT, "C": None, "D": LIMIT // 2}   # the bytes of the "fit" entries (C: the last U that fits)

# F. the shape table under the other forms: every H = 32 entry without the windowed sum under
# IGN_RESIDENT=2, and the batches under IGN_RES_GROUP=2 and 3 (qs_n17 with a second graph of its counts: a
# group of one graph has no boundary)
PG_SHAPES = sorted(n for n, s in sc.SHAPES.items() if s.hidden == 32 and not s.env)
GROUPED = {n: _c(*sc.SHAPES[n].graphs) for n in ("b15_1", "b16_16", "b17_15_32", "b_p1_between")}
GROUPED["qs_n17"] = _c(*sc.SHAPES["qs_n17"].graphs, G(20, 6, sc._rand(20, 4, 24), N=17, seed=1), **_Q)


def case(name):
    return CASES.get(name) or ROWS16.get(name) or GROUPED[name]


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(desc, dims, mi, plan, graphs, labels, parameters) of an entry, built once per session."""
    c = case(name)
    desc, dims = sc.model(c.kind, 32)
    graphs = [sc.graph(g, c.kind) for g in c.graphs]
    mi, plan, labels, prm = sc.inputs_for(desc, dims, graphs)
    return desc, dims, mi, plan, graphs, labels, prm


def case_expected(name, group=None):
    c = case(name)
    return expected(case_inputs(name)[4], c.kind, c.group if group is None else group)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle's predictions of an entry, read-only."""
    from oracle.dense_forward import DenseOracle
    desc, dims, _, _, graphs, _, prm = case_inputs(name)
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def grad_reference(name):
    """torch autograd of the float64 restatement on an entry: (loss, l2, {name: gradient}, predictions)."""
    from oracle.train_oracle import TorchOracle
    desc, dims, _, _, graphs, labels, prm = case_inputs(name)
    o = TorchOracle(desc, dims, prm).loss_and_grads(graphs, labels)
    sc.well_conditioned(labels, o[3])
    return o
