"""The graph-resident forward's set-up (resident.hip, in front of the first iteration): the [features | zeros]
states written as whole float4s, the sum MPs' CSR, the row order, the message rows and the step codes
copied as 16-byte vectors from wherever a graph's offset puts them, and the iteration-0 projection started
before the path states are there.  Predictions and every entity's final states bitwise those of the batched
launches (IGN_RESIDENT=0) on the same seeded graphs, on tiny graphs at that code's edges:

  feature width   a row's features fill part of one float4 column (1, 3), exactly one (4), one and a part
                  (5), every column (32); two source entities of different widths (Q-size)
  row counts      P = 1, 15, 16, 17 paths and U = 1, 16, 17 union rows: one item, and one short of, on and
                  one past the 16-row tile (128 float4 items: two waves of the 1024-thread trip)
  message counts  a link with 0, 7, 8, 9 and 67 messages; whole graphs of 7, 8 and 9 messages (less than,
                  exactly and one more than one 16-byte vector of 16-bit rows)
  batch layout    graphs of odd sizes in front, one workgroup per graph (IGN_RES_GROUP=1), so that a graph's
                  message rows, row order and step codes start at odd, 2-byte-aligned offsets
  forms           the default (all-LDS for these sizes), IGN_RESIDENT=2 (path states and step codes in global
                  memory), and the CSR-global form on resident_cases' Q-size graph of 260 union rows

and one training forward + backward (the SAVE form: the path loop is skipped, the copies are not): gradients
bitwise those of IGN_RESIDENT=0, as tests/test_gpu_widths.py holds the two training forwards to each other."""
import copy

import numpy as np
import pytest

from ignnition_amd.engine import Batch, Engine, MPPlan, device_count
from ignnition_amd.json_operations import Model_information
from tests import resident_cases as rc
from tests import shape_cases as sc
from tests.shape_cases import G
from tests.test_gpu_training import _engine_grads

pytestmark = pytest.mark.gpu

_ENV = ("IGN_RESIDENT", "IGN_RESIDENT_PG", "IGN_RES_GROUP", "IGN_RESIDENT_TRAIN")
_FEATURE = {"path": "traffic", "link": "link_capacity", "node": "queue_sizes"}
PG, ONE = {"IGN_RESIDENT": "2"}, {"IGN_RES_GROUP": "1"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _inputs(kind, specs, widths):
    """(desc, dims, plan, graphs, labels, parameters): shape_cases' graphs with each entity's feature redrawn
    at widths[entity] columns (uniform in [-1, 1), seeded per graph and entity)."""
    desc, dims = sc.model(kind, 32)
    dims = dict(dims, **{_FEATURE[e]: w for e, w in widths.items()})
    graphs = []
    for n, spec in enumerate(specs):
        g = dict(sc.graph(spec, kind))
        for k, (e, w) in enumerate(sorted(widths.items())):
            rng = np.random.default_rng(1000 * n + k)
            g[_FEATURE[e]] = rng.uniform(-1, 1, int(g["num_" + e]) * w).astype(np.float32)
        graphs.append(g)
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    return desc, dims, plan, graphs, sc.labels_for(graphs), plan.init_params(sc.SEED, bias_scale=sc.BIAS)


def _forward(monkeypatch, plan, prm, graphs, env):
    """Predictions (direct, then replayed from the captured hipGraph: equal), every entity's final states
    and resident_info of a fresh engine under env."""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    out = b.forward().reshape(-1).copy()
    for _ in range(2):
        np.testing.assert_array_equal(b.forward().reshape(-1), out)
    states = {e: b.state(e) for e in plan.entities}
    info = b.resident_info()
    b.close()
    eng.close()
    return out, states, info


def _check(monkeypatch, kind, specs, widths, envs, form=None):
    _, _, plan, graphs, _, prm = _inputs(kind, specs, widths)
    ref, ref_states, info = _forward(monkeypatch, plan, prm, graphs, {"IGN_RESIDENT": "0"})
    assert info["active"] == 0 and np.all(np.isfinite(ref))
    for env in envs:
        out, states, info = _forward(monkeypatch, plan, prm, graphs, env)
        assert info["active"] == 1, (env, info)
        if env.get("IGN_RESIDENT") == "2":
            assert info["form"] >= 1, info
        else:   # the default env on these sizes: the all-LDS form, unless the case names another
            assert info["form"] == (form or 0), info
        if "IGN_RES_GROUP" in env:
            assert info["workgroups"] == len(graphs), info
        np.testing.assert_array_equal(out, ref, err_msg=str(env))
        for e in plan.entities:
            assert states[e].shape == ref_states[e].shape
            np.testing.assert_array_equal(states[e], ref_states[e], err_msg="%s %s" % (env, e))


# two graphs of odd sizes: 17 paths over 5 links (a second float4 trip's worth of neither), 15 over 3
_PAIR = (G(17, 5, sc._rand(17, 3, 40)), G(15, 3, sc._rand(15, 2, 41), seed=1))


@pytest.mark.parametrize("link_f", [1, 5])
@pytest.mark.parametrize("path_f", [1, 3, 4, 5, 32])
def test_feature_widths(monkeypatch, path_f, link_f):
    _check(monkeypatch, "routenet", _PAIR, {"path": path_f, "link": link_f}, [ONE, dict(ONE, **PG)])


@pytest.mark.parametrize("link_f,node_f", [(1, 5), (5, 1)])
def test_two_source_entities_of_different_widths(monkeypatch, link_f, node_f):
    """Q-size: the union rows' entity select (links, then nodes from row 5 / row 3 on, inside a float4 trip)."""
    specs = (G(17, 5, sc._rand(17, 3, 42), N=3), G(9, 3, sc._rand(9, 2, 43), N=2, seed=1))
    _check(monkeypatch, "qsize", specs, {"path": 3, "link": link_f, "node": node_f}, [ONE, dict(ONE, **PG), {}])


ROWS = {
    "p1_u1": G(1, 1, 1),
    "p15_u16": G(15, 16, 2),
    "p16_u17": G(16, 17, 2),
    "p17_u1": G(17, 1, 1),
    "p17_u16": G(17, 16, 2),
    "p16_u16": G(16, 16, 1),
}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_row_counts(monkeypatch, name):
    _check(monkeypatch, "routenet", (ROWS[name],), {"path": 5, "link": 3}, [{}, PG])


def test_row_counts_in_one_batch(monkeypatch):
    """Every row-count graph in one batch, one workgroup each and under the automatic grouping."""
    specs = tuple(ROWS[n] for n in sorted(ROWS))
    _check(monkeypatch, "routenet", specs, {"path": 5, "link": 3}, [ONE, dict(ONE, **PG), {}])


_ODD = G(3, 2, (1, 2, 2), seed=9)    # 5 messages, 2 union rows, 15 step codes in front of the next graph


@pytest.mark.parametrize("hot", [0, 7, 8, 9, 67])
def test_message_counts_of_a_link(monkeypatch, hot):
    """Link 0 with ``hot`` messages (0: idle) in a graph behind an odd one."""
    specs = (_ODD, G(80, 4, sc._rand(80, 3, 50 + hot), hot=hot, seed=hot))
    _check(monkeypatch, "routenet", specs, {"path": 1, "link": 1}, [ONE, dict(ONE, **PG)])


@pytest.mark.parametrize("m", [7, 8, 9, 67])
def test_message_counts_of_a_graph(monkeypatch, m):
    """A graph of m messages in all (m one-link paths over one link), behind an odd one and in front of
    another: the message rows' vector copy with no, one or eight whole vectors, head and tail."""
    specs = (_ODD, G(m, 1, 1, seed=m), G(5, 2, (1, 2, 1, 1, 2), seed=2))
    _check(monkeypatch, "routenet", specs, {"path": 1, "link": 1}, [ONE, dict(ONE, **PG), {}])


def test_idle_link_last(monkeypatch):
    specs = (_ODD, G(40, 15, sc._rand(40, 3, 6), idle_links=1, seed=3))
    _check(monkeypatch, "routenet", specs, {"path": 3, "link": 5}, [ONE, dict(ONE, **PG)])


def test_csr_global_form(monkeypatch):
    """resident_cases' Q-size graph past edge B (260 union rows: the message rows stay in L2) behind an odd
    graph, features of 5, 3 and 1 columns."""
    big = rc.CASES["e_b_over"].graphs[0]
    specs = (G(3, 2, (1, 2, 2), N=2, seed=9), big)
    _check(monkeypatch, "qsize", specs, {"path": 5, "link": 3, "node": 1}, [ONE], form=2)


def test_training_forward_and_backward(monkeypatch):
    """forward_train + backward on a tiny RouteNet batch: one resident launch, and the gradient bits of
    the per-MP training forward under IGN_RESIDENT=0."""
    desc, dims, plan, graphs, labels, prm = _inputs("routenet", (_ODD,) + _PAIR, {"path": 5, "link": 3})
    runs = {}
    for v in ("1", "0"):
        for k in _ENV:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("IGN_RESIDENT", v)
        monkeypatch.setenv("IGN_RES_GROUP", "1")
        eng = Engine(plan, 0)
        eng.set_params(prm)
        eng.set_timing(True)
        eng, b, pred, loss, _, grads = _engine_grads(desc, dims, graphs, labels, prm, eng)
        assert eng.stats()["mp_resident"]["launches"] == int(v)
        runs[v] = (np.asarray(pred).reshape(-1).copy(), loss, grads.cpu().numpy())
        b.close()
        eng.close()
    assert np.abs(runs["0"][2]).sum() > 0
    np.testing.assert_array_equal(runs["1"][0], runs["0"][0])
    assert runs["1"][1] == runs["0"][1]
    np.testing.assert_array_equal(runs["1"][2], runs["0"][2])
