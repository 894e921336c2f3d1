"""The graph-resident ign_forward leaves out the last iteration's updates that nothing reads
(MPP::dead_in_last_iter; IGN_DEAD_LAST=0: every update runs) and ign_batch_state runs them on demand:
predictions and every entity's final states bitwise those of IGN_DEAD_LAST=0 and of the batched launches
(IGN_RESIDENT=0, which run every update under both switch values), in each of the resident forward's
forms, direct and replayed from the captured hipGraph, for
T = 1 (the last iteration is the first), T = 2 and the configs' T = 8, with link counts on and off the
16-row tile.  The statistics count what ran: the left-out launches are missing from a forward and appear
once when a state is read."""

import copy

import numpy as np
import pytest

from ignnition_amd import model_examples, synthetic, workloads
from ignnition_amd.engine import Batch, Engine, MPPlan
from ignnition_amd.json_operations import Model_information

pytestmark = pytest.mark.gpu


def _model(kind, T, links=False):
    desc = (model_examples.qsize if kind == "qsize" else model_examples.routenet)(iterations=T)
    if links:   # predict on the links: their last update is read, nothing is left out
        desc["readout"][0]["input"] = ["link"]
    _, dims, _ = workloads.model(kind)
    return Model_information(copy.deepcopy(desc), dims)


def _graphs(mi, kind, spec):
    """spec: (topology, n) or a list of (nodes, undirected links) per graph."""
    if isinstance(spec, tuple):
        samples = [synthetic.routenet_sample(spec[0], 70 + g, qsize=kind == "qsize") for g in range(spec[1])]
    else:
        samples = [synthetic.routenet_sample(graph_id=80 + g, qsize=kind == "qsize", n_nodes=n, n_links=m)
                   for g, (n, m) in enumerate(spec)]
    return workloads.graph_inputs(mi, samples)[0]


def _run(monkeypatch, plan, prm, graphs, dead, env, n_dead, resident):
    """One engine under IGN_DEAD_LAST=dead and env: the predictions of a direct and of replayed forwards
    (all bitwise equal, checked here), every entity's states read in the orders the reader must serve
    (equal, checked here), and the launch counts that show what ran."""
    monkeypatch.setenv("IGN_DEAD_LAST", dead)
    for k in ("IGN_RESIDENT", "IGN_RESIDENT_PG", "IGN_RES_GROUP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n_sum = sum(m["aggr"] == "sum" for m in plan.mps)
    skipped = n_dead if dead == "1" and resident else 0   # the batched launches run every update
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    info = b.resident_info()
    assert info["active"] == int(resident), info
    eng.set_timing(True)
    timed = b.forward().copy()                               # timed forwards launch directly
    st = eng.stats()
    assert st["mp_resident"]["launches"] == int(resident)
    assert st["sum_gru"]["launches"] == (0 if resident else n_sum * plan.iterations), st["sum_gru"]
    s_a = {e: b.state(e) for e in plan.entities}              # forward, state
    assert eng.stats()["sum_gru"]["launches"] == st["sum_gru"]["launches"] + skipped   # each left-out update, now
    s_b = {e: b.state(e) for e in plan.entities}              # a state read twice
    assert eng.stats()["sum_gru"]["launches"] == st["sum_gru"]["launches"] + skipped   # ... and only once
    eng.set_timing(False)
    first = b.forward().copy()                                # the hipGraph is captured here and replayed
    second = b.forward().copy()
    s_c = {e: b.state(e) for e in plan.entities}              # forward, forward, state
    third = b.forward().copy()                                # a replay after a finished entity changed its slot
    s_d = {e: b.state(e) for e in plan.entities}
    for o in (first, second, third):
        np.testing.assert_array_equal(o, timed)
    for s in (s_b, s_c, s_d):
        for e in plan.entities:
            np.testing.assert_array_equal(s[e], s_a[e], err_msg=e)
    b.close()
    eng.close()
    return timed, s_a, info


CASES = {
    # all-LDS form; two graphs: the auto rule runs both in one workgroup (K = 2); 42 links each
    "routenet-nsfnet2-T1": ("routenet", 1, ("nsfnet", 2), {}, 0),
    "routenet-nsfnet2-T2": ("routenet", 2, ("nsfnet", 2), {}, 0),
    "routenet-nsfnet2-T8": ("routenet", 8, ("nsfnet", 2), {}, 0),
    # GEANT2 x3 (74 links): all-LDS one graph per workgroup, and the global-path form forced
    "routenet-geant2-T8": ("routenet", 8, ("geant2", 3), {}, 0),
    "routenet-geant2-pg-T1": ("routenet", 1, ("geant2", 3), {"IGN_RESIDENT": "2"}, 1),
    "routenet-geant2-pg-T2": ("routenet", 2, ("geant2", 3), {"IGN_RESIDENT": "2"}, 1),
    "routenet-geant2-pg-T8": ("routenet", 8, ("geant2", 3), {"IGN_RESIDENT": "2"}, 1),
    # the headline's own form: one synth50 graph's path states do not fit LDS
    "routenet-synth50-T8": ("routenet", 8, ("synth50", 1), {}, 1),
    # Q-size: two source entities, both updates dead, tiles of two entities
    "qsize-nsfnet2-T1": ("qsize", 1, ("nsfnet", 2), {"IGN_RESIDENT_PG": "1"}, 0),
    "qsize-nsfnet2-T8": ("qsize", 8, ("nsfnet", 2), {"IGN_RESIDENT_PG": "1"}, 0),
    "qsize-nsfnet2-pg-T2": ("qsize", 2, ("nsfnet", 2), {"IGN_RESIDENT": "2"}, 1),
    "qsize-synth50-csr-T8": ("qsize", 8, ("synth50", 1), {}, 2),   # its sum CSR is read from L2 too
    # exactly 16 links (one full tile) alone, and beside a graph of 14 (one workgroup, 30 rows)
    "routenet-16links-T8": ("routenet", 8, [(7, 8)], {}, 0),
    "routenet-16+14links-T2": ("routenet", 2, [(7, 8), (6, 7)], {}, 0),
    "routenet-16links-pg-T8": ("routenet", 8, [(7, 8)], {"IGN_RESIDENT": "2"}, 1),
    "qsize-16links-T2": ("qsize", 2, [(7, 8)], {}, 0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_dead_last_updates_are_skipped_and_finished_on_demand(monkeypatch, case):
    kind, T, spec, env, form = CASES[case]
    mi = _model(kind, T)
    plan = MPPlan.from_model_info(mi)
    assert plan.iterations == T
    n_dead = sum(plan.dead_in_last_iter())
    assert n_dead == (2 if kind == "qsize" else 1)
    graphs = _graphs(mi, kind, spec)
    if not isinstance(spec, tuple):
        assert len(graphs[0]["link_capacity"]) == 16
    prm = plan.init_params(7, bias_scale=0.1)
    runs = {}
    for dead in ("1", "0"):
        for route in ("resident", "batched"):
            e = dict(env) if route == "resident" else {"IGN_RESIDENT": "0"}
            runs[dead, route] = _run(monkeypatch, plan, prm, graphs, dead, e, n_dead, route == "resident")
    out, states, _ = runs["0", "batched"]
    assert np.all(np.isfinite(out))
    for key, (o, s, _) in runs.items():
        np.testing.assert_array_equal(o, out, err_msg=str(key))
        for e in plan.entities:
            np.testing.assert_array_equal(s[e], states[e], err_msg="%s %s" % (key, e))
    on, off = runs["1", "resident"][2], runs["0", "resident"][2]
    assert on["form"] == off["form"] == form, (on, off)
    # the cost model counts what runs: one of the T sum updates less
    assert on["flops"] < off["flops"] and on["bytes_stage"] < off["bytes_stage"] and on["mfma_bf16"] < off["mfma_bf16"]
    assert on["tile_steps"] == off["tile_steps"] and on["bytes_compulsory"] == off["bytes_compulsory"]
    if form:
        assert on["bytes_roundtrip"] < off["bytes_roundtrip"]


@pytest.mark.parametrize("env", [{}, {"IGN_RESIDENT": "2"}], ids=["lds", "pg"])
def test_read_links_and_nothing_is_skipped(monkeypatch, env):
    """RouteNet predicting on the links: no update is dead, so both switch values run the same launches
    and give the same bits (_run's launch counts expect no left-out update)."""
    mi = _model("routenet", 3, links=True)
    plan = MPPlan.from_model_info(mi)
    assert plan.dead_in_last_iter() == [False, False]
    graphs = _graphs(mi, "routenet", ("nsfnet", 2))
    prm = plan.init_params(7, bias_scale=0.1)
    runs = [_run(monkeypatch, plan, prm, graphs, dead, e, 0, e is env)
            for dead in ("1", "0") for e in (env, {"IGN_RESIDENT": "0"})]
    for o, s, _ in runs[1:]:
        np.testing.assert_array_equal(o, runs[0][0])
        for e in plan.entities:
            np.testing.assert_array_equal(s[e], runs[0][1][e])
    assert runs[0][2] == runs[2][2]   # the resident cost model does not move with the switch
