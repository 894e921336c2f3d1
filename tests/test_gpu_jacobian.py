"""Batch.forward_tangents (ign_forward_jacobian, jacobian.hip): K feature directions through one linearised
forward, against float64 autograd J.v_k of the restated model with the feature columns as leaves (the
reference of tests/test_gpu_tangent.py: the reverse passes of all predictions, then a product per direction).

Every case: T = 2, init_params(SEED, bias_scale=BIAS), the graphs and K of tests/test_gpu_scenarios.py's
table plus one reset_after cell with options from tests/gru_cases.py; direction k standard normal over every
feature of every entity from default_rng(100 + k).  Bounds: dpred[k] within 1e-4
relative L2 of J.v_k over the batch, pred within TOL max(1, |ref|) of the float64 forward."""
import copy
import functools

import numpy as np
import pytest
import torch

from ignnition_amd import workloads
from ignnition_amd._lib import EngineError
from ignnition_amd.engine import Batch, Engine, MPPlan, device_count
from ignnition_amd.generate_model import ComnetModel
from ignnition_amd.json_operations import Model_information
from tests import gru_cases, layernorm_cases
from tests import shape_cases as sc
from tests import test_gpu_scenarios as ts
from tests.input_grad_oracle import CellInputGradOracle
from tests.test_gpu_parity import TOL
from tests.test_gpu_tangent import _rel
from tests.test_gpu_widths import _same_bits

pytestmark = pytest.mark.gpu
OPTIONS = "rn_hard_sigmoid"   # recurrent_activation hard_sigmoid, reset_after true; its first NSFNET sample


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(desc, dims, plan, graphs, parameters, {entity: {feature: [K, rows of the batch, size]}})."""
    if name == OPTIONS:
        desc, dims, _, plan, graphs, _, prm = gru_cases.case_inputs(name)
        graphs, K = graphs[:1], 17
    else:
        desc, dims, plan, graphs, prm, _ = ts._inputs(name)
        K = ts.CASES[name][4]
    rngs = [np.random.default_rng(100 + k) for k in range(K)]
    v = {ent: {f: np.stack([r.standard_normal((sum(int(g["num_" + ent]) for g in graphs), size)).astype(np.float32)
                            for r in rngs]) for f, size in fs} for ent, fs in zip(plan.entities, plan.features) if fs}
    return desc, dims, plan, graphs, prm, v


def _only(v, k):
    """Direction k alone, as forward_tangent takes it."""
    return {e: {f: a[k] for f, a in fs.items()} for e, fs in v.items()}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(float64 predictions, J.v_k [K, predictions]); read-only."""
    desc, dims, _, graphs, prm, v = _inputs(name)
    o = CellInputGradOracle(desc, dims, prm)
    pred = o.forward(graphs)
    leaves, parts = [], []
    for ent, feats in v.items():
        r0 = 0
        for gi, g in enumerate(graphs):
            n = int(g["num_" + ent])
            for f, a in feats.items():
                leaves.append(o.leaves[gi][f])
                parts.append(a[:, r0:r0 + n].astype(np.float64))
            r0 += n
    rows = torch.autograd.grad(pred, leaves, torch.eye(pred.numel(), dtype=pred.dtype), allow_unused=True, is_grads_batched=True)
    jv = sum(np.einsum("krs,prs->kp", p, g.numpy()) for g, p in zip(rows, parts) if g is not None)
    out = pred.detach().numpy(), jv
    for a in out:
        a.setflags(write=False)
    return out


def _run(name, v=None, count=None):
    desc, dims, _, graphs, prm, own = _inputs(name)
    eng, b = ts._open(desc, dims, graphs, prm)
    out = b.forward_tangents(own if v is None else v, directions_count=count)
    b.close()
    eng.close()
    return out


@pytest.mark.parametrize("name", sorted(ts.CASES) + [OPTIONS])
def test_against_float64_autograd(name):
    ref, jv = _reference(name)
    pred, dpred = _run(name)
    assert dpred.shape == jv.shape + (1,) and np.all(np.linalg.norm(jv, axis=1) > 0)
    errs = [_rel(dpred[k], jv[k]) for k in range(len(jv))]
    print("%s: K %d, %d predictions, worst dpred relative L2 %.3g, pred max scaled error %.3g"
          % (name, len(jv), ref.size, max(errs), (np.abs(pred.reshape(-1) - ref) / np.maximum(1, np.abs(ref))).max()))
    assert max(errs) <= 1e-4
    assert np.all(np.abs(pred.reshape(-1) - ref) <= TOL * np.maximum(1, np.abs(ref)))


@pytest.mark.parametrize("name", ["s17", "qsize"])
def test_a_directions_bits_are_its_own_and_the_single_pass_agrees(name):
    """Neither K nor the index of a direction in its block reaches its bits; pred is forward_tangent's, bit for
    bit, and dpred[k] its dpred to rounding (the accumulation structure differs)."""
    desc, dims, _, graphs, prm, v = _inputs(name)
    pred, full = _run(name)
    moved = _run(name, {e: {f: np.roll(a, 5, axis=0) for f, a in fs.items()} for e, fs in v.items()})[1]
    np.testing.assert_array_equal(moved, np.roll(full, 5, axis=0))
    eng, b = ts._open(desc, dims, graphs, prm)
    for k in (0, 15, 16):
        one = b.forward_tangents({e: {f: a[k:k + 1] for f, a in fs.items()} for e, fs in v.items()})[1]
        np.testing.assert_array_equal(one[0], full[k], err_msg="direction %d alone" % k)
        pred1, single = b.forward_tangent(_only(v, k))
        np.testing.assert_array_equal(pred, pred1)
        print("%s: direction %d against forward_tangent, relative L2 %.3g" % (name, k, _rel(full[k], single.astype(np.float64).reshape(-1))))
        assert _rel(full[k], single.astype(np.float64).reshape(-1)) <= 1e-4
    b.close()
    eng.close()


def test_zero_and_doubled_directions_and_an_untouched_batch():
    desc, dims, plan, graphs, prm, v = _inputs("qsize")
    eng, b = ts._open(desc, dims, graphs, prm)
    before = (b.forward().copy(), {e: b.state(e) for e in plan.entities})
    pred, dpred = b.forward_tangents(v)
    pred0, dpred0 = b.forward_tangents({}, directions_count=3)
    _, dpred2 = b.forward_tangents({e: {f: 2 * a for f, a in fs.items()} for e, fs in v.items()})
    _same_bits((b.forward(), {e: b.state(e) for e in plan.entities}), before, "after forward_tangents")
    b.close()
    eng.close()
    assert dpred0.shape[0] == 3 and np.all(dpred0 == 0) and np.array_equal(pred0, pred)
    assert np.any(dpred != 0) and np.array_equal(dpred2, 2 * dpred)   # a power of two commutes with every rounding


def test_poisoned_scratch(monkeypatch):
    """NaN-filled scratch blocks (IGN_POOL_POISON=1): no padding row and no unwritten block reaches a result."""
    clean = _run("qsize")
    monkeypatch.setenv("IGN_POOL_POISON", "1")
    for a, c in zip(_run("qsize"), clean):
        np.testing.assert_array_equal(a, c)


def _refusals():
    for r in ts._refusals():
        yield ("reset_after = false",) + r[1:] + ({},) if r[0] == "cell with options" else r + ({},)
    desc = layernorm_cases.width_model(16)
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), sc.dims("routenet")))
    yield "LayerNormalization", desc, sc.dims("routenet"), [sc.graph(ts._P17)], plan.init_params(sc.SEED, bias_scale=sc.BIAS), {}
    desc, dims, mi, graphs, _ = workloads.make_synthetic_inputs(n_nodes=60, hidden=32, iterations=2, window=8)
    yield "halo rows", desc, dims, graphs, MPPlan.from_model_info(mi).init_params(3, bias_scale=0.1), {"halo_rows": {"node": 1}}


@pytest.mark.parametrize("what", ["attention", "convolution", "concat on axis 2", "message network", "readout operation",
                                  "LayerNormalization", "reset_after = false", "128/128", "halo rows", "training step"])
def test_refused_by_name(what):
    _, desc, dims, graphs, prm, kw = next(r for r in _refusals() if r[0] == what)
    eng = Engine(MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)), 0)
    eng.set_params(prm)
    b = Batch(eng, graphs, **kw)
    if what == "training step":
        b.enable_training()
        b.forward_train()
    before = None if kw else b.forward().copy()   # (a batch with halo rows forwards in steps, with its neighbours)
    with pytest.raises(EngineError, match="forward jacobian: .*" + what) as e:
        b.forward_tangents({}, directions_count=2)
    assert e.value.code == -2
    if before is not None:
        np.testing.assert_array_equal(b.forward(), before)
    b.close()
    eng.close()


def test_argument_errors_and_the_model_level_call():
    desc, dims, plan, graphs, prm, v = _inputs("s17")
    eng, b = ts._open(desc, dims, graphs, prm)
    traffic, cap = v["path"]["traffic"], v["link"]["link_capacity"]
    for bad, text in [({"path": traffic, "link": cap[:16]}, "directions"), ({"path": traffic[:, :-1]}, "forward_tangents: .*shape"),
                      ({"router": traffic}, "no entity"), ({}, "directions")]:
        with pytest.raises(ValueError, match=text):
            b.forward_tangents(bad)
    pred, dpred = b.forward_tangents(v)
    b.close()
    eng.close()
    model = ComnetModel(Model_information(copy.deepcopy(desc), dims), params=prm)
    both = model.jacobian(graphs, {"traffic": traffic, "link_capacity": cap})
    assert np.array_equal(both[0], pred) and np.array_equal(both[1], dpred)
    only = model.jacobian(graphs, {"traffic": traffic})   # a feature left out does not move
    assert np.array_equal(only[0], pred) and only[1].shape == dpred.shape and not np.array_equal(only[1], dpred)
    with pytest.raises(ValueError, match="unknown feature"):
        model.jacobian(graphs, {"delay": traffic})
    model.engine.close()
