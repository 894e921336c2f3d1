"""tests/readout_op_cases.py against its own arrays and against the float64 oracles (no GPU).

Every count an entry states is recomputed; DenseOracle and TorchOracle agree on every entry to 1e-10; and
the table bites: a float64 restatement with one of the faults a pooling / product kernel can have moves a
prediction by at least 10 x TOL (scaled as test_gpu_parity's _close scales it) or a gradient tensor by at
least 10 x GTOL (relative L2, as test_gpu_training's _check_grads measures it).  That is the condition under
which the bounds tests/test_gpu_readout_ops.py applies mean something on these shapes.

Which entries a perturbation is applied to follows from its operation (PERTURBATIONS below): a tie split
needs a max pooling with a stated tie, a broadcast operand from the graph before needs a product of a graph
tensor with a row tensor in a batch of more than one graph.  Among those, at most one entry in ten is exempt
(EXEMPT), each with its reason."""
import time

import numpy as np
import pytest
import torch

from oracle.train_oracle import _T, TorchOracle
from tests import readout_op_cases as rc

from tests.test_gpu_parity import TOL          # importing them needs the built library, not a GPU
from tests.test_gpu_training import GTOL
_TIMES = {}


def _batch_rows(graphs, key):
    return [int(g[key]) for g in graphs]


# ---------------------------------------------------------------------------------------------
# the counts
@pytest.mark.parametrize("name", rc.ALL)
def test_counts(name):
    c, cnt = rc.CASES[name], rc.counts(name)
    _, _, _, plan, graphs, labels, prm = rc.case_inputs(name)
    assert len(graphs) == len(c.graphs)
    sp = rc.spaces(c)
    pools = [o for o in c.ops if o["type"] == "pooling"]
    if pools:
        s = sp[pools[0]["input"][0]]
        rows = tuple(1 if s == "graph" else len(g["src_adj_paths_links"]) if s == "adj" else
                     int(g["num_" + s])
                     for g in graphs)
        assert cnt["rows"] == rows
        assert cnt["chunks"] == tuple((n + 4095) // 4096 for n in rows)
    for e, idle in cnt.get("no_edge", ()):
        key, ent = ("src_adj_paths_links", "path") if e == 0 else ("dst_adj_paths_links", "link")
        off, got = 0, []
        for g in graphs:
            deg = np.bincount(np.asarray(g[key], np.int64), minlength=int(g["num_" + ent]))
            got += [int(off + r) for r in np.flatnonzero(deg == 0)]
            off += int(g["num_" + ent])
        assert tuple(got) == tuple(idle), "%s rows of the batch that no edge reads" % ent
    if "stride" in cnt:
        assert cnt["stride"] == sum(_batch_rows(graphs[:1], "num_path")) * rc.widths(name)["pe"] > rc.GRID_CAP
        assert sum(len(g["src_adj_paths_links"]) for g in graphs) * rc.widths(name)["ep"] > rc.GRID_CAP
    assert [l.size for l in labels] == [rc.pred_rows(c, g) * (rc.predict_width(name) if c.predict == "identity" else 1)
                                        for g in graphs]
    if c.zero_gru:
        for g in graphs:
            n, t = int(g["num_path"]), np.asarray(g["traffic"])
            sr = rc.special_rows(n)
            assert np.all(np.abs(t[sr]) >= 32) and np.abs(np.delete(t, sr)).max(initial=0) < 1
            assert t.argmax() == sr[-1] and (n == 1 or t.argmin() == sr[-2])


def test_axes_are_covered():
    """The issue's axes, read back from the table."""
    W = {n: rc.widths(n) for n in rc.ALL}
    pooled = {W[n][o["input"][0]] for n in rc.ALL for o in rc.CASES[n].ops if o["type"] == "pooling"}
    assert {1, 3, 16, 32, 48, 255, 256, 257, 300} <= pooled
    rows = {r for n in rc.POOLING for r in rc.counts(n)["rows"]}
    assert {1, 2, 255, 256, 257, 4095, 4096, 4097, 8193} <= rows
    assert {1, 2, 3, 5, 64} <= {len(rc.CASES[n].graphs) for n in rc.ALL}
    assert rc.counts("rows4097")["rows"] == (4097, 17) and rc.counts("rows4097")["chunks"] == (2, 1)
    assert {rc.counts(n)["ties"][2][0] for n in rc.TIES} >= {2, 17, 4097}
    prod = {W[n][o["output_name"]] for n in rc.ALL for o in rc.CASES[n].ops if o["type"] == "product"}
    assert {1, 16, 48, 300} <= prod
    cat = {sum(W[n][i] for i in o["input"]) for n in rc.ALL for o in rc.CASES[n].ops if o["type"] == "neural_network"}
    assert {33, 17} <= cat and rc.predict_width("three_consumers") == 32 + 1 + 48
    assert set(rc.BITWISE) <= set(rc.ALL)


# ---------------------------------------------------------------------------------------------
# the two oracles
@pytest.mark.parametrize("name", rc.ALL)
def test_oracles_agree(name):
    t0 = time.perf_counter()
    ref = rc.reference(name)
    t1 = time.perf_counter()
    loss, _, grads, pred = rc.grad_reference(name)
    _TIMES[name] = (t1 - t0, time.perf_counter() - t1)
    print("%s: DenseOracle %.2f s, TorchOracle with autograd %.2f s" % ((name,) + _TIMES[name]))
    assert np.abs(ref.reshape(-1) - pred).max() <= 1e-10 * max(1.0, np.abs(pred).max())
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())


def test_stride_case_is_well_conditioned_in_float32():
    """The largest entry: plain float32 autograd of the same restatement is within GTOL / 10 of float64 on every
    gradient tensor, so that GTOL on the GPU measures the kernels and not the entry's conditioning."""
    import oracle.train_oracle as to
    desc, dims, _, _, graphs, labels, prm = rc.case_inputs("stride")
    _, _, g64, _ = rc.grad_reference("stride")
    o = TorchOracle(desc, dims, prm)
    o.p = {k: torch.tensor(np.asarray(v, np.float32), dtype=torch.float32, requires_grad=True) for k, v in prm.items()}
    to._T = torch.float32
    try:
        _, _, g32, _ = o.loss_and_grads(graphs, labels)
    finally:
        to._T = torch.float64
    assert all(v.dtype == torch.float32 and v.grad.dtype == torch.float32 for v in o.p.values() if v.grad is not None)
    rel = {k: (np.linalg.norm(g32[k].astype(np.float64) - g64[k]) - 1e-7) / np.linalg.norm(g64[k]) for k in g64}
    assert max(np.linalg.norm(g32[k].astype(np.float64) - g64[k]) for k in g64) > 0, "not a float32 run"
    print("float32 autograd vs float64, worst tensor: %s %.3g" % max((v, k) for k, v in rel.items())[::-1])
    assert max(rel.values()) <= GTOL / 10


@pytest.mark.parametrize("name", rc.TIES)
def test_ties_and_their_analytic_gradient(name):
    """The stated multiplicity, in the float64 oracle's tensors; for the zero-GRU entries the tie column's
    bias gradient is the sum over graphs of dL/d(prediction) of that column, its kernel gradient that times
    the mean state of the graph's rows (column 0: traffic / 4)."""
    c = rc.CASES[name]
    desc, dims, _, _, graphs, labels, prm = rc.case_inputs(name)
    out, col, mult = rc.counts(name)["ties"]
    o = _Perturbed(desc, dims, prm, None)
    o.forward(graphs)
    for g, m in enumerate(mult):
        v, y = o.seen[g][[op for op in c.ops if op.get("output_name") == out][0]["input"][0]], o.seen[g][out]
        assert int((v[:, col] == y[0, col]).sum()) == m
    if c.zero_gru:
        db, dk = rc.analytic_tie_gradient(name)
        _, _, grads, _ = rc.grad_reference(name)
        np.testing.assert_allclose(grads[rc.op_param(0, 0, "bias")][col], db, rtol=1e-12)
        np.testing.assert_allclose(grads[rc.op_param(0, 0, "kernel")][:, col], dk, rtol=1e-12, atol=1e-18)
        assert abs(db) > 1e-3 and abs(dk[0]) > 1e-6


# ---------------------------------------------------------------------------------------------
# bite
class _Perturbed(TorchOracle):
    """TorchOracle with one fault in its pooling / product restatement (``mut``; None: none).  The tensors
    of the neighbouring graphs come from a clean pass (detached)."""

    def __init__(self, desc, dims, prm, mut):
        super().__init__(desc, dims, prm)
        self.mut, self.seen, self.clean, self.g = mut, {}, None, 0

    def forward(self, graphs):
        if self.mut in ("next_first", "bcast_prev") and self.clean is None:
            with torch.no_grad():
                o = _Perturbed(self.d, self.dims, {k: v.detach().numpy() for k, v in self.p.items()}, None)
                o.forward(graphs)
            self.clean = o.seen
        out = []
        for self.g, x in enumerate(graphs):
            out.append(self.forward_graph(x).reshape(-1))
        self.G = len(graphs)
        return torch.cat(out)

    def _readout(self, state, x):
        var = dict(state)
        gspace = set()
        self.seen[self.g] = var
        m, g = self.mut, self.g
        for counter, op in enumerate(self.d["readout"]):
            t = op["type"]
            if t in ("predict", "neural_network"):
                h = torch.cat([var[i] for i in op["input"]], 1)
                for layer, pre in self._layers(op, counter):
                    h = h @ self.p[pre + "/kernel"]
                    if pre + "/bias" in self.p:
                        h = h + self.p[pre + "/bias"]
                    h = _act(h, layer.get("activation"))
                if t == "predict":
                    return h
                var[op["output_name"]] = h
                if op["input"][0] in gspace:
                    gspace.add(op["output_name"])
            elif t == "pooling":
                v = var[op["input"][0]]
                n = v.shape[0]
                if m == "drop_last" and op["input"][0] not in gspace:   # the last row of every chunk
                    keep = np.ones(n, bool)
                    keep[[r for r in range(n) if (r + 1) % rc.POOL_CHUNK == 0 or r == n - 1]] = False
                    v = v[torch.as_tensor(keep)] if keep.any() else v * 0
                if m == "next_first" and op["input"][0] not in gspace and g + 1 in self.clean:
                    v = torch.cat([v, self.clean[g + 1][op["input"][0]][:1]], 0)
                kind = op["type_pooling"]
                if kind == "sum":
                    r = v.sum(0)
                elif kind == "mean":
                    r = v.sum(0) / (n + (1 if m == "count_plus" else -1 if m == "count_minus" and n > 1 else 0))
                else:
                    ind = (v == v.max(0).values).to(_T)
                    r = (v * ind).sum(0) / ind.sum(0)
                    if m == "full_tie":   # the value of the maximum, the whole gradient on every tied row
                        r = (v * ind).sum(0) - (ind.sum(0) - 1) * r.detach()
                var[op["output_name"]] = r.reshape(1, -1)
                gspace.add(op["output_name"])
            elif t == "product":
                a, b = (var[i] for i in op["input"])
                ag, bg = (i in gspace for i in op["input"])
                if m == "bcast_prev" and ag != bg and g > 0:
                    if ag:
                        a = self.clean[g - 1][op["input"][0]]
                    else:
                        b = self.clean[g - 1][op["input"][1]]
                o = a * b
                if m == "w1_col0" and o.shape[1] > 1 and 1 in (a.shape[1], b.shape[1]) and a.shape[1] != b.shape[1]:
                    w, wide = (a, b) if a.shape[1] == 1 else (b, a)
                    wd = w.detach()   # same values; the width-1 operand's gradient from column 0 only
                    o = wide * wd + torch.cat([wide.detach()[:, :1] * (w - wd), torch.zeros_like(wide[:, 1:])], 1)
                var[op["output_name"]] = o
                if ag and bg:
                    gspace.add(op["output_name"])
            else:
                if m == "gather_shift":   # every edge reads the source row before its own (row 0: the last)
                    x = dict(x)
                    x["src_" + op["adj_list"]] = (np.asarray(x["src_" + op["adj_list"]], np.int64) - 1) % var[op["input"][0]].shape[0]
                var[op["output_name_src"]] = var[op["input"][0]][torch.as_tensor(np.asarray(x["src_" + op["adj_list"]], np.int64))]
                var[op["output_name_dst"]] = var[op["input"][1]][torch.as_tensor(np.asarray(x["dst_" + op["adj_list"]], np.int64))]
        raise AssertionError("no predict")


from oracle.train_oracle import _act  # noqa: E402


def _has(name, pred):
    return any(pred(o) for o in rc.CASES[name].ops)


def _bcast(name):
    c, sp = rc.CASES[name], rc.spaces(rc.CASES[name])
    return len(c.graphs) > 1 and any(o["type"] == "product" and (sp[o["input"][0]] == "graph") != (sp[o["input"][1]] == "graph")
                                     for o in c.ops)


def _w1(name):
    w = rc.widths(name)
    return any(o["type"] == "product" and w[o["output_name"]] > 1 and w[o["input"][1]] == 1 for o in rc.CASES[name].ops)


def _pool_rows(name):
    sp = rc.spaces(rc.CASES[name])
    return any(o["type"] == "pooling" and sp[o["input"][0]] != "graph" for o in rc.CASES[name].ops)


# perturbation -> the entries whose operations it applies to
PERTURBATIONS = {
    "drop_last": [n for n in rc.ALL if _pool_rows(n)],
    "next_first": [n for n in rc.ALL if _pool_rows(n) and len(rc.CASES[n].graphs) > 1],
    "count_plus": list(rc.MEAN),
    "count_minus": list(rc.MEAN),
    "full_tie": list(rc.TIES),
    "bcast_prev": [n for n in rc.ALL if _bcast(n)],
    "w1_col0": [n for n in rc.ALL if _w1(n)],
    # (a pooling does not see the order of its rows: entries whose ep is read by poolings alone are not meant)
    "gather_shift": [n for n in rc.EXTEND if max(int(g["num_path"]) for g in rc.case_inputs(n)[4]) > 1 and
                     ("ep" in rc.CASES[n].pin or _has(n, lambda o: o["type"] != "pooling" and "ep" in o["input"]))],
}
# (perturbation, entry): why it cannot move this entry
EXEMPT = {
    ("drop_last", "ext_max_ep"): "the last edge row repeats a path row that an earlier edge row holds too: the maximum and "
                                 "the share of each path stay (the tie split covers this entry)",
    ("count_minus", "pool_pool"): "its mean is over a graph tensor: count 1, and count - 1 divides by 0",
}


def _moved(name, mut):
    """(largest scaled prediction change / TOL, largest relative gradient change / GTOL) of a perturbation."""
    desc, dims, _, _, graphs, labels, prm = rc.case_inputs(name)
    _, _, g0, p0 = rc.grad_reference(name)
    _, _, g1, p1 = _Perturbed(desc, dims, prm, mut).loss_and_grads(graphs, labels)
    dp = (np.abs(p1 - p0) / np.maximum(1.0, np.abs(p0))).max() / TOL
    dg = max((np.linalg.norm(g1[k] - g0[k]) - 1e-7) / max(np.linalg.norm(g0[k]), 1e-30) for k in g0) / GTOL
    return dp, dg


@pytest.mark.parametrize("mut,name", [(m, n) for m in PERTURBATIONS for n in PERTURBATIONS[m]])
def test_perturbation_moves_the_reference(mut, name):
    if (mut, name) in EXEMPT:
        assert max(_moved(name, mut)) < 10.0, "exempt, but it bites: take it off the list"
        return
    dp, dg = _moved(name, mut)
    print("%s on %s: predictions %.3g x TOL, worst gradient tensor %.3g x GTOL" % (mut, name, dp, dg))
    assert max(dp, dg) >= 10.0


def test_exemptions_are_few():
    assert set(m for m, _ in EXEMPT) <= set(PERTURBATIONS)
    for m, names in PERTURBATIONS.items():
        ex = [n for mm, n in EXEMPT if mm == m]
        assert set(ex) <= set(names) and 10 * len(ex) <= len(names), m


def test_the_unperturbed_restatement_is_the_oracle():
    for name in ("g5", "prod_w48", "tie17", "ext_idle"):
        assert max(_moved(name, None)) <= 0.0
