"""tests/aggregation_cases.py holds what its comments claim (CPU, numpy on the built arrays, no engine):
the attention groups' cell and empty-cell counts, the block edge of n_groups, the two-message cell, link
0's in-degree and the idle row of the convolution cases, the logit ranges of the float64 oracle, and
finite, well-conditioned references for every case."""
import copy
import ctypes as C
import json

import numpy as np
import pytest

from ignnition_amd import _lib
from ignnition_amd.engine import MPPlan
from ignnition_amd.json_operations import Model_information
from tests import aggregation_cases as ac
from tests import shape_cases as sc


def _graphs(name):
    c = ac.CASES[name]
    return c, [sc.graph(g, c.kind) for g in c.graphs]


def test_the_table_covers_the_issue():
    assert {c.hidden for n, c in ac.CASES.items() if n in ac.ATTENTION} == {16, 32}
    assert {c.hidden for n, c in ac.CASES.items() if n in ac.CONVOLUTION} == {16, 32}
    assert {(dict(c.aggr)["concat_axis"], c.hidden) for n, c in ac.CASES.items() if n in ac.CONCAT} == \
        {(a, h) for a in (1, 2) for h in (16, 32, 64)}
    acts = {dict(ac.CASES[n].aggr).get("activation_function", "relu") for n in ac.CONVOLUTION if n in ac.GRADS}
    assert acts == {"relu", "tanh", "selu"}
    assert {ac.CASES[n].deg0 for n in ac.CONVOLUTION} >= {1, 3, 4, 5, 64}
    assert {ac.CASES[n].mod4 for n in ac.BATCHES if n in ac.ATTENTION} >= {0, 1, 3}
    assert "logit_overflow" not in ac.GRADS and "logit_moderate" in ac.GRADS
    for n, c in ac.CASES.items():
        rows = max(int(g[k]) for g in _graphs(n)[1] for k in ("num_path", "num_link"))
        assert rows <= 300, n


@pytest.mark.parametrize("name", ac.ATTENTION)
def test_attention_groups(name):
    """The (graph, position) groups recomputed from dst_adj_* / seq_*: the stated cells and empty cells of
    every group, n_groups mod 4, and whether a cell holds two messages."""
    c, graphs = _graphs(name)
    per = [ac.groups(c.kind, g) for g in graphs]
    assert tuple(tuple(q[0] for q in g) for g in per) == c.cells
    assert tuple(tuple(q[1] for q in g) for g in per) == c.empty
    assert sum(len(g) for g in per) % 4 == c.mod4
    assert (max(q[2] for g in per for q in g) == 2) == c.dup
    if c.kind == "routenet":   # group q holds the links of more than q messages (positions without holes)
        for spec, g, cells in zip(c.graphs, graphs, c.cells):
            if "link_positions" not in dict(spec):
                deg = np.bincount(g["dst_adj_paths_links"], minlength=int(g["num_link"]))
                assert cells == tuple(int((deg > q).sum()) for q in range(deg.max()))


def test_attention_edges_named_by_the_issue():
    first = {n: ac.CASES[n].cells[0][0] for n in ("att_l1", "att_l63", "att_l64", "att_l65", "att_l129")}
    assert first == {"att_l1": 1, "att_l63": 63, "att_l64": 64, "att_l65": 65, "att_l129": 129}
    for n in ("att_l65", "att_l129"):   # one hot link: the later groups are small and hold empties
        c = ac.CASES[n]
        assert all(1 <= k <= 3 for k in c.cells[0][1:]) and all(e > 0 for e in c.empty[0][1:])
    assert 0 in ac.CASES["att_hole"].cells[0] and sum(len(g) for g in ac.CASES["att_hole"].cells) <= 8   # one block
    assert all(e > 0 for e in ac.CASES["att_idle"].empty[0])
    assert [ac.CASES["qatt_p%d" % p].cells[0][0] for p in (1, 16, 17, 64, 65)] == [1, 16, 17, 64, 65]
    for p in (16, 17, 64, 65):   # late positions: one path, P - 1 empties
        c = ac.CASES["qatt_p%d" % p]
        assert c.cells[0][-1] == 1 and c.empty[0][-1] == p - 1


@pytest.mark.parametrize("name", [n for n in ac.CONVOLUTION if ac.CASES[n].kind == "routenet"])
def test_convolution_degrees(name):
    c, graphs = _graphs(name)
    deg = np.bincount(graphs[0]["dst_adj_paths_links"], minlength=int(graphs[0]["num_link"]))
    if c.deg0 is not None:
        assert deg[0] == c.deg0
    if c.idle is not None:
        assert deg[c.idle] == 0 and np.count_nonzero(deg == 0) == 1
        assert c.idle not in graphs[0]["src_adj_links_paths"]   # no path reads the idle link
    else:
        assert deg.min() >= 1
    if name.startswith("conv_l"):   # the link rows at the 16-row tile
        assert len(deg) == int(name[6:])


def test_logit_ranges():
    """From the float64 oracle's scores (every attention MP run of the case, before the max is taken)."""
    scores = ac.reference("logit_moderate")[2]
    top = max(np.abs(s).max() for s in scores)
    print("logit_moderate: largest |e| %.3g" % top)
    assert 5 <= top <= 15
    scores = ac.reference("logit_overflow")[2]
    hi, lo = max(s.max() for s in scores), min(s.min() for s in scores)
    print("logit_overflow: e in [%.4g, %.4g]" % (lo, hi))
    assert hi >= 90 and lo <= -90
    with np.errstate(over="ignore"):
        assert np.exp(np.float32(hi)) == np.inf   # what a softmax without its max would compute
    assert any(e > 0 for e in ac.CASES["logit_overflow"].empty[0])
    # a group without empty cells whose every score is <= -90: exp(e) is 0 in float32 unless the group's own
    # maximum is subtracted (the second graph's groups hold one cell each)
    lone = [float(s[0, q]) for s in scores if s.shape[0] == 1 for q in range(s.shape[1])]
    print("logit_overflow: the one-cell groups' scores", np.round(lone, 1))
    assert ac.CASES["logit_overflow"].empty[1] == (0, 0, 0) and min(lone) <= -90 and np.exp(np.float32(min(lone))) < 1.2e-38


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_oracle_health(name):
    c = ac.CASES[name]
    pred, states, _ = ac.reference(name)
    assert np.isfinite(pred).all() and (pred.size == 1 or np.ptp(pred) > 1e-4)
    if c.idle is None:
        for e, s in states.items():
            assert np.isfinite(s).all(), e
    else:   # only the idle link's state is non-finite
        assert np.isnan(states["link"][c.idle]).all()
        assert np.isfinite(np.delete(states["link"], c.idle, axis=0)).all() and np.isfinite(states["path"]).all()
    labels = ac.case_inputs(name)[5]
    if c.grads:
        o_g, o_pred = ac.grad_reference(name)[2:]
        np.testing.assert_allclose(o_pred, pred, rtol=1e-9, atol=1e-12)
        sc.well_conditioned(labels, o_pred)
        bad = sorted(n for n, g in o_g.items() if not np.isfinite(g).all())
        # degree 0: autograd carries the idle link's NaN into its own update cell's tensors and nowhere else
        assert bad == (sorted("link_update/" + t for t in ("bias", "kernel", "recurrent_kernel")) if c.idle is not None else [])


@pytest.mark.parametrize("name", sorted(ac.REFUSED_H64))
def test_hidden_64_is_refused_by_both_front_ends(name):
    """Attention and convolution have kernels for 16 and 32 units: ign_plan_create (the Python lowering's
    descriptor) and ign_plan_create_json refuse 64 with the same status and text, and leave no plan."""
    kind, aggr, code, text = ac.REFUSED_H64[name]
    desc, dims = ac.model(kind, aggr, 64)
    d, keep = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)).to_desc()
    hp = C.c_void_p()
    rc = _lib.lib.ign_plan_create(C.byref(d), 0, C.byref(hp))
    from_python = _lib.lib.ign_last_error().decode()
    assert rc == code and not hp, from_python
    assert text in from_python
    hj = C.c_void_p()
    rc = _lib.lib.ign_plan_create_json(json.dumps(desc).encode(), json.dumps(dims).encode(), 0, C.byref(hj))
    from_json = _lib.lib.ign_last_error().decode()
    assert rc == code and not hj, from_json
    assert from_json == from_python


@pytest.mark.parametrize("name", sorted(n for n, c in ac.CASES.items() if c.hidden != 32))
def test_other_hidden_sizes_are_lowered(name):
    desc, dims, _, plan, _, _, _ = ac.case_inputs(name)
    d, keep = plan.to_desc()
    h = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create(C.byref(d), 0, C.byref(h)))
    _lib.lib.ign_plan_destroy(h)
