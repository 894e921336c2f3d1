"""Batch.scenario_parameter_gradients (ign_backward_scenarios_params, scenario_wgrad.hip): the parameter
gradients of sum_s cot_s . pred_s over S feature sets on one topology in one pass, against float64 autograd run
once per scenario on the graphs with that scenario's features substituted and summed over the scenarios.

Cases, inputs and cotangents are tests/test_gpu_scenarios.py's and tests/test_gpu_scenario_gradients.py's.
Bound per parameter tensor: |got - want| <= GTOL |want| + 1e-7 (L2), the project's bound for every gradient
against float64 (tests/test_gpu_training.py); pred within TOL max(1, |ref|) of the float64 forward."""
import copy
import functools

import numpy as np
import pytest
import torch

from ignnition_amd import generate_model
from ignnition_amd._lib import EngineError
from ignnition_amd.engine import device_count
from ignnition_amd.generate_model import ComnetModel
from ignnition_amd.json_operations import Model_information
from tests import test_gpu_scenarios as ts
from tests.input_grad_oracle import CellInputGradOracle
from tests.test_gpu_parity import TOL
from tests.test_gpu_scenario_gradients import _cot
from tests.test_gpu_training import GTOL
from tests.test_gpu_widths import _same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(float64 predictions [S, predictions], {parameter name: gradient summed over the scenarios}), read-only."""
    desc, dims, _, _, prm, _ = ts._inputs(name)
    o = CellInputGradOracle(desc, dims, prm)
    preds, total = [], {k: np.zeros(tuple(v.shape)) for k, v in o.p.items()}
    for s, w in enumerate(_cot(name)):
        pred = o.forward(ts._scenario_graphs(name, s))
        g = torch.autograd.grad((pred.reshape(-1) * torch.tensor(w, dtype=pred.dtype)).sum(), list(o.p.values()), allow_unused=True)
        for k, gi in zip(o.p, g):
            if gi is not None:
                total[k] += gi.numpy()
        preds.append(pred.detach().numpy().reshape(-1))
    for a in total.values():
        a.setflags(write=False)
    return np.stack(preds), total


def _rel(got, want):
    return {k: np.linalg.norm(got[k].astype(np.float64) - v) / max(np.linalg.norm(v), 1e-30) for k, v in want.items()}


def _run(name, feats=None, w=None):
    desc, dims, _, graphs, prm, own = ts._inputs(name)
    eng, b = ts._open(desc, dims, graphs, prm)
    out = b.scenario_parameter_gradients(own if feats is None else feats, _cot(name) if w is None else w)
    b.close()
    eng.close()
    return out


@pytest.mark.parametrize("name", sorted(ts.CASES))
def test_against_float64_autograd(name):
    """Measured on the MI355X (worst tensor's relative L2): see DESIGN.md §3q's table."""
    ref, want = _reference(name)
    assert all(np.linalg.norm(v) > 0 for v in want.values())   # a pass that returns zeros cannot succeed
    pred, got = _run(name)
    assert sorted(got) == sorted(want) and all(got[k].shape == v.shape and got[k].dtype == np.float32 for k, v in want.items())
    rel = _rel(got, want)
    print("%s: S %d, %d tensors, worst %s relative L2 %.3g, pred max scaled error %.3g"
          % ((name, len(ref), len(want)) + max((v, k) for k, v in rel.items())[::-1] + (ts._scaled_err(pred, ref),)))
    for k, v in want.items():
        assert np.linalg.norm(got[k].astype(np.float64) - v) <= GTOL * np.linalg.norm(v) + 1e-7, "%s: rel err %.3g" % (k, rel[k])
    assert pred.shape == ref.shape + (1,) and np.all(np.abs(pred[:, :, 0] - ref) <= TOL * np.maximum(1, np.abs(ref)))


@pytest.mark.parametrize("name", ["s17", "qsize"])
def test_bits_and_invariants(name, monkeypatch):
    desc, dims, plan, graphs, prm, feats = ts._inputs(name)
    w = _cot(name)
    eng, b = ts._open(desc, dims, graphs, prm)
    before = (b.forward().copy(), {e: b.state(e) for e in plan.entities})
    pred, full = b.scenario_parameter_gradients(feats, w)
    np.testing.assert_array_equal(pred, b.forward_scenarios(feats))
    _same_bits(b.scenario_parameter_gradients(feats, w), (pred, full), "a second call")
    assert all(np.any(g != 0) for g in full.values())
    assert all(np.all(g == 0) for g in b.scenario_parameter_gradients(feats, np.zeros_like(w))[1].values())
    # S = 17 is the first block plus the 17th scenario alone: the same sum in another order
    pick = lambda lo, hi: {e: {f: a[lo:hi] for f, a in fs.items()} for e, fs in feats.items()}   # noqa: E731
    head, tail = b.scenario_parameter_gradients(pick(0, 16), w[:16])[1], b.scenario_parameter_gradients(pick(16, 17), w[16:])[1]
    split = _rel({k: head[k] + tail[k] for k in full}, full)
    for env in ("IGN_SCEN_WGRAD_FUSED", "IGN_SCEN_GRAD_CHUNK_MIB"):   # the unfused form; one block per chunk: two chunks
        monkeypatch.setenv(env, "0")
        other = b.scenario_parameter_gradients(feats, w)
        monkeypatch.delenv(env)
        np.testing.assert_array_equal(other[0], pred)
        split = {k: max(v, _rel(other[1], full)[k]) for k, v in split.items()}
    print("%s: blocks apart / unfused / one-block chunks against the default, worst relative L2 %.3g" % (name, max(split.values())))
    assert max(split.values()) <= 1e-5
    _same_bits((b.forward(), {e: b.state(e) for e in plan.entities}), before, "after scenario_parameter_gradients")
    b.close()
    eng.close()
    monkeypatch.setenv("IGN_POOL_POISON", "1")   # NaN-filled scratch: no padding row and no unwritten block reaches a result
    _same_bits(_run(name), (pred, full), "poisoned scratch")


@pytest.mark.parametrize("what", [r[0] for r in ts._refusals()])
def test_refused_by_name(what):
    _, desc, dims, graphs, prm = next(r for r in ts._refusals() if r[0] == what)
    eng, b = ts._open(desc, dims, graphs, prm)
    if what == "training step":
        b.enable_training()
        b.forward_train()
    before = b.forward().copy()
    with pytest.raises(EngineError, match="scenario parameter gradients: .*" + what) as e:
        b.scenario_parameter_gradients({}, scenarios=2)
    assert e.value.code == -2
    np.testing.assert_array_equal(b.forward(), before)
    b.close()
    eng.close()


def test_argument_errors():
    desc, dims, _, graphs, prm, feats = ts._inputs("s17")
    w = _cot("s17")
    eng, b = ts._open(desc, dims, graphs, prm)
    traffic, cap = feats["path"]["traffic"], feats["link"]["link_capacity"]
    for bad, cot, text in [({"path": traffic, "link": cap[:16]}, None, "scenarios"), ({"router": traffic}, None, "no entity"),
                           ({"path": traffic[:, :-1]}, None, "scenario_gradients: .*shape"), ({}, None, "scenarios"),
                           (feats, w[0], "scenario_gradients: cotangents .*shape"), (feats, w[:, :-1], "scenario_gradients: cotangents .*shape")]:
        with pytest.raises(ValueError, match=text):
            b.scenario_parameter_gradients(bad, cot)
    b.close()
    eng.close()


def test_model_level_call_normalises(monkeypatch):
    desc, dims, _, graphs, prm, feats = ts._inputs("s17")
    desc = copy.deepcopy(desc)
    for e in desc["entities"]:
        for f in e["features"]:
            if f["name"] == "traffic":
                f["normalization"] = "halve"
    monkeypatch.setitem(generate_model.user_namespace, "halve", lambda x, name: x * np.float32(0.5))
    model = ComnetModel(Model_information(desc, dims), params=prm)
    raw, w = feats["path"]["traffic"], _cot("s17")
    got = model.scenario_parameter_gradients(graphs, {"traffic": raw}, dpred=w)
    b = model.batch(graphs)
    want = b.scenario_parameter_gradients({"path": {"traffic": raw * np.float32(0.5)}}, w)
    b.close()
    _same_bits(got, want, "scenario_parameter_gradients")
    model.engine.close()
