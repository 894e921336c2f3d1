"""Batch.scenario_gradients (ign_backward_scenarios, scenario_adjoint.hip): the input gradients of S feature
sets on one topology in one pass, against float64 autograd run once per scenario on the graphs with that
scenario's features substituted (tests/input_grad_oracle.py, the feature columns as leaves).

Every case: tests/test_gpu_scenarios.py's table with its inputs; scenario s's cotangent standard normal over
the predictions from default_rng(300 + s).  Bounds: scenario s's gradient within
1e-4 relative L2 over every feature value of every entity, pred within TOL max(1, |ref|) of the float64 forward."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ignnition_amd import generate_model
from ignnition_amd._lib import EngineError, lib
from ignnition_amd.engine import MPPlan, device_count
from ignnition_amd.generate_model import ComnetModel
from ignnition_amd.json_operations import Model_information
from tests import test_gpu_scenarios as ts
from tests.input_grad_oracle import CellInputGradOracle
from tests.test_gpu_adjoint import _flat
from tests.test_gpu_parity import TOL
from tests.test_gpu_tangent import _rel
from tests.test_gpu_widths import _same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _cot(name):
    """[S, predictions], read-only."""
    n = ts._reference(name).shape[1]
    w = np.stack([np.random.default_rng(300 + s).standard_normal(n).astype(np.float32) for s in range(ts.CASES[name][4])])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(float64 predictions [S, predictions], gradients [S, every feature value of every entity in plan order])."""
    desc, dims, _, _, prm, _ = ts._inputs(name)
    o = CellInputGradOracle(desc, dims, prm)
    preds, grads = [], []
    for s, w in enumerate(_cot(name)):
        pred = o.forward(ts._scenario_graphs(name, s))
        leaves = [l[f["name"]] for ent in o.d["entities"] for f in ent["features"] for l in o.leaves]
        g = torch.autograd.grad((pred.reshape(-1) * torch.tensor(w, dtype=pred.dtype)).sum(), leaves, allow_unused=True)
        grads.append(np.concatenate([(torch.zeros_like(l) if gi is None else gi).numpy().reshape(-1) for gi, l in zip(g, leaves)]))
        preds.append(pred.detach().numpy().reshape(-1))
    out = np.stack(preds), np.stack(grads)
    for a in out:
        a.setflags(write=False)
    return out


def _sub(feats, pick):
    return {e: {f: pick(a) for f, a in fs.items()} for e, fs in feats.items()}


def _run(name, feats=None, w=None):
    desc, dims, plan, graphs, prm, own = ts._inputs(name)
    eng, b = ts._open(desc, dims, graphs, prm)
    pred, grads = b.scenario_gradients(own if feats is None else feats, _cot(name) if w is None else w)
    b.close()
    eng.close()
    return pred, _flat(plan, grads)


@pytest.mark.parametrize("name", sorted(ts.CASES))
def test_against_float64_autograd(name):
    ref, want = _reference(name)
    assert np.all(np.linalg.norm(want, axis=1) > 0)   # a pass that returns zeros cannot succeed
    pred, got = _run(name)
    errs = [_rel(got[s], want[s]) for s in range(len(want))]
    print("%s: S %d, %d predictions, %d feature values, worst scenario relative L2 %.3g, pred max scaled error %.3g"
          % (name, len(want), ref.shape[1], want.shape[1], max(errs), ts._scaled_err(pred, ref)))
    assert got.shape == want.shape and max(errs) <= 1e-4
    assert pred.shape == ref.shape + (1,) and np.all(np.abs(pred[:, :, 0] - ref) <= TOL * np.maximum(1, np.abs(ref)))


@pytest.mark.parametrize("name", ["s17", "qsize"])
def test_a_scenarios_bits_are_its_own_and_the_batch_is_untouched(name, monkeypatch):
    desc, dims, plan, graphs, prm, feats = ts._inputs(name)
    w = _cot(name)
    eng, b = ts._open(desc, dims, graphs, prm)
    before = (b.forward().copy(), {e: b.state(e) for e in plan.entities})
    pred, full = b.scenario_gradients(feats, w)
    full = _flat(plan, full)
    np.testing.assert_array_equal(pred, b.forward_scenarios(feats))
    for k in (0, 15, 16):
        one = b.scenario_gradients(_sub(feats, lambda a: a[k:k + 1]), w[k:k + 1])
        np.testing.assert_array_equal(one[0][0], pred[k], err_msg="scenario %d alone: pred" % k)
        np.testing.assert_array_equal(_flat(plan, one[1])[0], full[k], err_msg="scenario %d alone" % k)
    moved = b.scenario_gradients(_sub(feats, lambda a: np.roll(a, 5, axis=0)), np.roll(w, 5, axis=0))
    np.testing.assert_array_equal(_flat(plan, moved[1]), np.roll(full, 5, axis=0))
    assert np.any(full != 0) and np.all(_flat(plan, b.scenario_gradients(feats, np.zeros_like(w))[1]) == 0)
    monkeypatch.setenv("IGN_SCEN_GRAD_CHUNK_MIB", "0")   # one block per chunk: two chunks here
    chunked = b.scenario_gradients(feats, w)
    monkeypatch.delenv("IGN_SCEN_GRAD_CHUNK_MIB")
    np.testing.assert_array_equal(chunked[0], pred)
    np.testing.assert_array_equal(_flat(plan, chunked[1]), full, err_msg="one-block chunks")
    _same_bits((b.forward(), {e: b.state(e) for e in plan.entities}), before, "after scenario_gradients")
    b.close()
    eng.close()
    monkeypatch.setenv("IGN_POOL_POISON", "1")   # NaN-filled scratch: no padding row and no unwritten block reaches a result
    poisoned = _run(name)
    np.testing.assert_array_equal(poisoned[0], pred)
    np.testing.assert_array_equal(poisoned[1], full)


def test_one_scenario_of_the_batchs_values_agrees_with_the_one_point_pass():
    desc, dims, plan, graphs, prm, _ = ts._inputs("qsize")
    w = _cot("qsize")[:1]
    eng, b = ts._open(desc, dims, graphs, prm)
    got = _flat(plan, b.scenario_gradients({}, w, scenarios=1)[1])[0]
    want = _flat(plan, b.backward_cotangents(w)[1])[0]
    b.close()
    eng.close()
    print("qsize: S = 1 on the batch's values against backward_cotangents, relative L2 %.3g" % _rel(got, want))
    assert np.linalg.norm(want) > 0 and _rel(got, want) <= 1e-4   # (two primals of different arithmetic: not bitwise)


@pytest.mark.parametrize("what", ["attention", "convolution", "concat on axis 2", "message network", "readout operation",
                                  "cell with options", "128/128", "training step"])
def test_refused_by_name(what):
    _, desc, dims, graphs, prm = next(r for r in ts._refusals() if r[0] == what)
    eng, b = ts._open(desc, dims, graphs, prm)
    if what == "training step":
        b.enable_training()
        b.forward_train()
    before = b.forward().copy()
    with pytest.raises(EngineError, match="backward scenarios: .*" + what) as e:
        b.scenario_gradients({}, scenarios=2)
    assert e.value.code == -2
    np.testing.assert_array_equal(b.forward(), before)
    b.close()
    eng.close()


def test_argument_errors():
    desc, dims, plan, graphs, prm, feats = ts._inputs("s17")
    w = _cot("s17")
    eng, b = ts._open(desc, dims, graphs, prm)
    traffic, cap = feats["path"]["traffic"], feats["link"]["link_capacity"]
    for bad, text in [({"path": traffic, "link": cap[:16]}, "scenarios"), ({"path": traffic[:, :-1]}, "scenario_gradients: .*shape"),
                      ({"router": traffic}, "no entity"), ({}, "scenarios")]:
        with pytest.raises(ValueError, match=text):
            b.scenario_gradients(bad)
    for bad in (w[0], w[:16], w[:, :-1]):
        with pytest.raises(ValueError, match="scenario_gradients: cotangents .*shape"):
            b.scenario_gradients(feats, bad)
    b.close()
    eng.close()
    bare = copy.deepcopy(desc)   # the same model, its links without features
    bare["entities"][[e["name"] for e in bare["entities"]].index("link")]["features"] = []
    bare_plan = MPPlan.from_model_info(Model_information(copy.deepcopy(bare), dims))
    eng, b = ts._open(bare, dims, graphs, bare_plan.init_params(ts.sc.SEED, bias_scale=ts.sc.BIAS))
    with pytest.raises(ValueError, match="has no features"):
        b.scenario_gradients({"link": cap})
    assert sorted(b.scenario_gradients({"path": traffic}, w)[1]) == ["path"]
    E, cot = len(bare_plan.entities), np.ascontiguousarray(w[:2, :, None])
    bufs = [np.zeros((2, r, 4), np.float32) for r in b.rows]
    only_path = (C.c_void_p * E)(*[a.ctypes.data if fs else None for a, fs in zip(bufs, bare_plan.features)])
    every = (C.c_void_p * E)(*[a.ctypes.data for a in bufs])
    none = (C.c_void_p * E)()
    for n_scen, feat, n_ents, c, outs in [(0, none, E, cot.ctypes.data, only_path), (2, none, E, None, only_path),
                                          (2, none, E, cot.ctypes.data, None), (2, none, E + 1, cot.ctypes.data, only_path),
                                          (2, none, E, cot.ctypes.data, every), (2, every, E, cot.ctypes.data, only_path)]:
        assert lib.ign_backward_scenarios(b.handle, n_scen, feat, n_ents, c, None, outs) == -1
    assert lib.ign_backward_scenarios(None, 2, none, E, cot.ctypes.data, None, only_path) == -1
    assert lib.ign_backward_scenarios(b.handle, 2, none, E, cot.ctypes.data, None, only_path) == 0
    b.close()
    eng.close()


def test_model_level_call_normalises(monkeypatch):
    desc, dims, plan, graphs, prm, feats = ts._inputs("s17")
    desc = copy.deepcopy(desc)
    for e in desc["entities"]:
        for f in e["features"]:
            if f["name"] == "traffic":
                f["normalization"] = "halve"
    monkeypatch.setitem(generate_model.user_namespace, "halve", lambda x, name: x * np.float32(0.5))
    model = ComnetModel(Model_information(desc, dims), params=prm)
    raw, w = feats["path"]["traffic"], _cot("s17")
    pred, grads = model.scenario_sensitivities(graphs, {"traffic": raw}, dpred=w)
    b = model.batch(graphs)
    want = b.scenario_gradients({"path": {"traffic": raw * np.float32(0.5)}}, w)
    b.close()
    _same_bits((pred, {"grads": _flat(plan, grads)}), (want[0], {"grads": _flat(plan, want[1])}), "scenario_sensitivities")
    with pytest.raises(ValueError, match="scenario_sensitivities: unknown feature"):
        model.scenario_sensitivities(graphs, {"delay": raw})
    model.engine.close()
