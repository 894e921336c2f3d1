"""Batch.forward_scenarios (ign_forward_scenarios, scenario.hip): S feature sets on one topology in one pass,
against the float64 oracle run once per scenario on the graphs with that scenario's features substituted.

Every case: T = 2, init_params(SEED, bias_scale=BIAS), scenario s's features uniform in [-1, 1) from
default_rng(100 + s) for every feature of every entity.  The bound is the project's own: TOL = 1e-4 on
|engine - oracle| / max(1, |oracle|), and _ieee_tol for the sum of >= 64 float32 terms."""
import copy
import functools

import numpy as np
import pytest

from ignnition_amd import generate_model
from ignnition_amd._lib import EngineError
from ignnition_amd.engine import Batch, Engine, MPPlan, device_count
from ignnition_amd.generate_model import ComnetModel
from ignnition_amd.json_operations import Model_information
from oracle.dense_forward import DenseOracle
from tests import activation_cases, aggregation_cases, edge_param_cases, gru_cases, wide_cases
from tests import shape_cases as sc
from tests.shape_cases import G, _rand
from tests.test_gpu_parity import TOL, _close, _ieee_tol, _scaled_err
from tests.test_gpu_widths import _same_bits
from tests.width_cases import _set_widths

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


_P17 = G(17, 17, wide_cases._mixed(17, 12))     # lengths 1 .. 12 over 17 links: two 16-row tiles' worth of paths
_QS = G(20, 6, _rand(20, 4, 22), N=17)
CASES = {   # name: (model, link / node width, path width, graphs, S)
    "s1": ("routenet", 32, 32, (_P17,), 1),      # one real scenario in a block of 16
    "s16": ("routenet", 32, 32, (_P17,), 16),    # a full block
    "s17": ("routenet", 32, 32, (_P17,), 17),    # a second block with one real row
    "len1": ("routenet", 32, 32, (G(24, 7, 1),), 17),                                    # one step per sequence
    "idle2": ("routenet", 32, 32, (G(40, 15, _rand(40, 3, 6), idle_links=2),), 17),     # destinations without a message
    "hot70": ("routenet", 32, 32, (G(80, 4, _rand(80, 3, 12), hot=70),), 16),           # a sum of 70 terms
    "h16": ("routenet", 16, 16, (_P17,), 17), "h64": ("routenet", 64, 64, (_P17,), 17),  # U in LDS at 64
    "l16_p32": ("routenet", 16, 32, (_P17,), 17), "l32_p16": ("routenet", 32, 16, (_P17,), 17),   # DIN != H both ways
    "qsize": ("qsize", 32, 32, (_QS,), 17),      # interleave of two sources, multi rows, hole codes, two sum MPs
    "concat1": ("concat1", 32, 32, (_QS,), 17),  # concat on axis 1
    "batch2": ("routenet", 32, 32, (_P17, G(24, 7, 1, seed=1)), 17),                     # graph offsets in the flat layout
}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(desc, dims, plan, graphs, parameters, {entity: {feature: [S, rows of the batch, size]}})."""
    kind, link, path, specs, S = CASES[name]
    desc, dims = wide_cases.model(kind, 32)
    _set_widths(desc, link=link, node=link, path=path)
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    graphs = [sc.graph(g, "routenet" if kind == "routenet" else "qsize") for g in specs]
    rngs = [np.random.default_rng(100 + s) for s in range(S)]
    feats = {ent: {f: np.stack([r.uniform(-1, 1, (sum(int(g["num_" + ent]) for g in graphs), size)).astype(np.float32)
                                for r in rngs]) for f, size in fs}
             for ent, fs in zip(plan.entities, plan.features) if fs}
    return desc, dims, plan, graphs, plan.init_params(sc.SEED, bias_scale=sc.BIAS), feats


def _scenario_graphs(name, s):
    """The case's graph dicts with scenario s's feature arrays substituted."""
    _, _, plan, graphs, _, feats = _inputs(name)
    out, r0 = [], {ent: 0 for ent in feats}
    for g in graphs:
        g = dict(g)
        for ent, fs in feats.items():
            n = int(g["num_" + ent])
            for f, a in fs.items():
                g[f] = a[s, r0[ent]:r0[ent] + n].reshape(np.shape(g[f]))
            r0[ent] += n
        out.append(g)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, seed=sc.SEED):
    """The float64 oracle per scenario, [S, predictions]; read-only."""
    desc, dims, plan, _, prm, _ = _inputs(name)
    ora = DenseOracle(desc, dims, prm if seed == sc.SEED else plan.init_params(seed, bias_scale=sc.BIAS))
    ref = np.stack([np.concatenate([ora._readout(ora.final_states(g), g).reshape(-1) for g in _scenario_graphs(name, s)])
                    for s in range(CASES[name][4])])
    ref.setflags(write=False)
    return ref


def _open(desc, dims, graphs, prm):
    eng = Engine(MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)), 0)
    eng.set_params(prm)
    return eng, Batch(eng, graphs)


def _run(name, feats=None):
    desc, dims, _, graphs, prm, own = _inputs(name)
    eng, b = _open(desc, dims, graphs, prm)
    out = b.forward_scenarios(own if feats is None else feats)
    b.close()
    eng.close()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_oracle(name):
    desc, dims, plan, graphs, prm, _ = _inputs(name)
    ref, out = _reference(name), _run(name)
    assert out.shape == ref.shape + (1,)
    # the scenarios differ from each other and (S = 1) from the batch's own values: a pass that ignores feat cannot succeed
    own = DenseOracle(desc, dims, prm).forward(graphs)
    assert np.ptp(np.vstack([ref, own[None]]), axis=0).max() > 1e-3
    print("%s: S %d, %d predictions, max scaled error vs float64 oracle %.3g" % (name, ref.shape[0], ref.shape[1], _scaled_err(out, ref)))
    for s in range(ref.shape[0]):
        _close(out[s], ref[s], _ieee_tol(plan, _scenario_graphs(name, s), prm, ref[s]) if name == "hot70" else TOL)


@pytest.mark.parametrize("name", ["s17", "qsize"])
def test_a_scenarios_bits_are_its_own(name):
    """Neither S nor the index of a scenario in its block reaches its bits."""
    feats = _inputs(name)[5]
    full = _run(name)
    for k in (0, 15, 16):
        one = _run(name, {e: {f: a[k:k + 1] for f, a in fs.items()} for e, fs in feats.items()})
        np.testing.assert_array_equal(one[0], full[k], err_msg="scenario %d alone" % k)
    moved = _run(name, {e: {f: np.roll(a, 5, axis=0) for f, a in fs.items()} for e, fs in feats.items()})
    np.testing.assert_array_equal(moved, np.roll(full, 5, axis=0))


def test_default_features_live_parameters_and_an_untouched_batch():
    desc, dims, plan, graphs, prm, feats = _inputs("s17")
    eng, b = _open(desc, dims, graphs, prm)
    before = (b.forward().copy(), {e: b.state(e) for e in plan.entities})
    same = b.forward_scenarios({}, scenarios=3)
    own = {e: {f: np.stack([np.concatenate([np.asarray(g[f], np.float32).reshape(-1, size) for g in graphs])] * 3)
               for f, size in fs} for e, fs in zip(plan.entities, plan.features) if fs}
    assert same.shape[0] == 3 and np.array_equal(same[0], same[1]) and np.array_equal(same[0], same[2])
    np.testing.assert_array_equal(same, b.forward_scenarios(own))
    first = b.forward_scenarios(feats)
    _same_bits((b.forward(), {e: b.state(e) for e in plan.entities}), before, "after forward_scenarios")
    eng.set_params(plan.init_params(6, bias_scale=sc.BIAS))
    second = b.forward_scenarios(feats)
    b.close()
    eng.close()
    _close(first, _reference("s17"))
    _close(second, _reference("s17", 6))
    assert _scaled_err(second, _reference("s17")) > 100 * TOL


def test_poisoned_scratch(monkeypatch):
    """NaN-filled scratch blocks (IGN_POOL_POISON=1): no padding row and no unwritten block reaches a result."""
    clean = _run("qsize")
    monkeypatch.setenv("IGN_POOL_POISON", "1")
    np.testing.assert_array_equal(_run("qsize"), clean)


def _refusals():
    a = aggregation_cases.case_inputs
    yield "attention", a("att_l1")[0], a("att_l1")[1], a("att_l1")[4], a("att_l1")[6]
    yield "convolution", a("conv_deg1")[0], a("conv_deg1")[1], a("conv_deg1")[4], a("conv_deg1")[6]
    yield "concat on axis 2", a("cat2_p1")[0], a("cat2_p1")[1], a("cat2_p1")[4], a("cat2_p1")[6]
    desc, dims, graphs, _, prm = edge_param_cases.case_inputs("sum_p1_first")
    yield "message network", desc, dims, graphs, prm
    desc = activation_cases.no_normalization(activation_cases.readout_op_model("tanh"))
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), sc.dims("routenet")))
    yield "readout operation", desc, sc.dims("routenet"), [sc.graph(_P17)], plan.init_params(sc.SEED, bias_scale=sc.BIAS)
    g = gru_cases.case_inputs("rn_v1")
    yield "cell with options", g[0], g[1], g[4], g[6]
    w = wide_cases.case_inputs("p1_l1")
    yield "128/128", w[0], w[1], w[3], w[4]
    desc, dims, _, graphs, prm, _ = _inputs("s17")
    yield "training step", desc, dims, graphs, prm


@pytest.mark.parametrize("what", ["attention", "convolution", "concat on axis 2", "message network", "readout operation",
                                  "cell with options", "128/128", "training step"])
def test_refused_by_name(what):
    _, desc, dims, graphs, prm = next(r for r in _refusals() if r[0] == what)
    eng, b = _open(desc, dims, graphs, prm)
    if what == "training step":
        b.enable_training()
        b.forward_train()
    before = b.forward().copy()
    with pytest.raises(EngineError, match="forward scenarios: .*" + what):
        b.forward_scenarios({}, scenarios=2)
    np.testing.assert_array_equal(b.forward(), before)
    b.close()
    eng.close()


def test_argument_errors():
    desc, dims, plan, graphs, prm, feats = _inputs("s17")
    eng, b = _open(desc, dims, graphs, prm)
    traffic, cap = feats["path"]["traffic"], feats["link"]["link_capacity"]
    for bad, text in [({"path": traffic, "link": cap[:16]}, "scenarios"), ({"path": traffic[:, :-1]}, "forward_scenarios: .*shape"),
                      ({"router": traffic}, "no entity"), ({}, "scenarios")]:
        with pytest.raises(ValueError, match=text):
            b.forward_scenarios(bad)
    b.close()
    eng.close()
    bare = copy.deepcopy(desc)   # the same model, its links without features
    bare["entities"][[e["name"] for e in bare["entities"]].index("link")]["features"] = []
    bare_plan = MPPlan.from_model_info(Model_information(copy.deepcopy(bare), dims))
    eng, b = _open(bare, dims, graphs, bare_plan.init_params(sc.SEED, bias_scale=sc.BIAS))
    with pytest.raises(ValueError, match="has no features"):
        b.forward_scenarios({"link": cap})
    assert b.forward_scenarios({"path": traffic}).shape == (17, 17, 1)
    b.close()
    eng.close()


def test_model_level_call_normalises(monkeypatch):
    desc, dims, plan, graphs, prm, feats = _inputs("s17")
    desc = copy.deepcopy(desc)
    for e in desc["entities"]:
        for f in e["features"]:
            if f["name"] == "traffic":
                f["normalization"] = "halve"
    monkeypatch.setitem(generate_model.user_namespace, "halve", lambda x, name: x * np.float32(0.5))
    model = ComnetModel(Model_information(desc, dims), params=prm)
    raw = feats["path"]["traffic"]
    got = model.predict_scenarios(graphs, {"traffic": raw})
    b = model.batch(graphs)
    np.testing.assert_array_equal(got, b.forward_scenarios({"path": {"traffic": raw * np.float32(0.5)}}))
    b.close()
    with pytest.raises(ValueError, match="unknown feature"):
        model.predict_scenarios(graphs, {"delay": raw})
    model.engine.close()
