"""Batch.backward_cotangents (ign_backward_jacobian, adjoint.hip): K prediction cotangents through one adjoint
sweep of the linearised forward, against float64 autograd J^T.w_k of the restated model with the feature
columns as leaves (tests/input_grad_oracle.py; the full Jacobian once per case, then a product per cotangent).

Every case: T = 2, the graphs and K of tests/test_gpu_scenarios.py's table plus one reset_after cell with
options from tests/gru_cases.py; cotangent k standard normal over the predictions from default_rng(200 + k).
Bounds: row k within 1e-4 relative L2 of J^T.w_k over every feature of every entity,
pred within TOL max(1, |ref|) of the float64 forward."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ignnition_amd import generate_model
from ignnition_amd._lib import EngineError, lib
from ignnition_amd.engine import Batch, Engine, MPPlan, device_count
from ignnition_amd.generate_model import ComnetModel
from ignnition_amd.json_operations import Model_information
from tests import gru_cases
from tests import test_gpu_jacobian as tj
from tests import test_gpu_scenarios as ts
from tests.input_grad_oracle import CellInputGradOracle
from tests.test_gpu_parity import TOL
from tests.test_gpu_tangent import _rel
from tests.test_gpu_widths import _same_bits

pytestmark = pytest.mark.gpu
OPTIONS = "rn_hard_sigmoid"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(desc, dims, plan, graphs, parameters)."""
    if name == OPTIONS:
        desc, dims, _, plan, graphs, _, prm = gru_cases.case_inputs(name)
        return desc, dims, plan, graphs[:1], prm
    return ts._inputs(name)[:5]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(float64 predictions, J [predictions, every feature value of every entity in plan order]); read-only."""
    desc, dims, _, graphs, prm = _case(name)
    o = CellInputGradOracle(desc, dims, prm)
    pred = o.forward(graphs)
    leaves = [l[f["name"]] for ent in o.d["entities"] for f in ent["features"] for l in o.leaves]
    rows = torch.autograd.grad(pred, leaves, torch.eye(pred.numel(), dtype=pred.dtype), allow_unused=True, is_grads_batched=True)
    J = np.concatenate([(np.zeros((pred.numel(),) + tuple(l.shape)) if g is None else g.numpy()).reshape(pred.numel(), -1)
                        for g, l in zip(rows, leaves)], axis=1)
    out = pred.detach().numpy(), J
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """_case(name) + (cotangents [K, predictions],), read-only."""
    K = 17 if name == OPTIONS else ts.CASES[name][4]
    w = np.stack([np.random.default_rng(200 + k).standard_normal(_reference(name)[0].size).astype(np.float32) for k in range(K)])
    w.setflags(write=False)
    return _case(name) + (w,)


def _flat(plan, grads):
    """[K, every feature value], in _reference's column order."""
    return np.concatenate([grads[e][f].reshape(len(grads[e][f]), -1) for e, fs in zip(plan.entities, plan.features) for f, _ in fs],
                          axis=1).astype(np.float64)


def _run(name, w=None):
    desc, dims, plan, graphs, prm, own = _inputs(name)
    eng, b = ts._open(desc, dims, graphs, prm)
    pred, grads = b.backward_cotangents(own if w is None else w)
    b.close()
    eng.close()
    return pred, _flat(plan, grads)


@pytest.mark.parametrize("name", sorted(ts.CASES) + [OPTIONS])
def test_against_float64_autograd(name):
    (ref, J), w = _reference(name), _inputs(name)[5]
    want = w.astype(np.float64) @ J
    assert np.all(np.linalg.norm(want, axis=1) > 0)   # a pass that returns zeros cannot succeed
    pred, got = _run(name)
    errs = [_rel(got[k], want[k]) for k in range(len(w))]
    print("%s: K %d, %d predictions, %d feature values, worst row relative L2 %.3g, pred max scaled error %.3g"
          % (name, len(w), ref.size, J.shape[1], max(errs), (np.abs(pred.reshape(-1) - ref) / np.maximum(1, np.abs(ref))).max()))
    assert got.shape == want.shape and max(errs) <= 1e-4
    assert np.all(np.abs(pred.reshape(-1) - ref) <= TOL * np.maximum(1, np.abs(ref)))


@pytest.mark.parametrize("name", ["s17", "qsize"])
def test_one_hot_cotangents_are_jacobian_rows(name):
    J = _reference(name)[1]
    picks = [0, 15, 16, len(J) - 1]
    got = _run(name, np.eye(len(J), dtype=np.float32)[picks])[1]
    errs = [_rel(got[k], J[i]) for k, i in enumerate(picks)]
    print("%s: rows %s, relative L2 %s" % (name, picks, ["%.3g" % e for e in errs]))
    assert np.all(np.linalg.norm(J[picks], axis=1) > 0) and max(errs) <= 1e-4


@pytest.mark.parametrize("name", ["s17", "qsize"])
def test_a_cotangents_bits_are_its_own_and_the_batch_is_untouched(name, monkeypatch):
    desc, dims, plan, graphs, prm, w = _inputs(name)
    eng, b = ts._open(desc, dims, graphs, prm)
    before = (b.forward().copy(), {e: b.state(e) for e in plan.entities})
    pred, full = b.backward_cotangents(w)
    full = _flat(plan, full)
    for k in (0, 15, 16):
        np.testing.assert_array_equal(_flat(plan, b.backward_cotangents(w[k:k + 1])[1])[0], full[k], err_msg="cotangent %d alone" % k)
    np.testing.assert_array_equal(_flat(plan, b.backward_cotangents(np.roll(w, 5, axis=0))[1]), np.roll(full, 5, axis=0))
    assert np.any(full != 0) and np.all(_flat(plan, b.backward_cotangents(np.zeros_like(w))[1]) == 0)
    np.testing.assert_array_equal(_flat(plan, b.backward_cotangents(2 * w)[1]), 2 * full)   # a power of two commutes with every rounding
    np.testing.assert_array_equal(pred, b.forward_tangents({}, directions_count=1)[0])
    _same_bits((b.forward(), {e: b.state(e) for e in plan.entities}), before, "after backward_cotangents")
    b.close()
    eng.close()
    monkeypatch.setenv("IGN_POOL_POISON", "1")   # NaN-filled scratch: no padding row and no unwritten block reaches a result
    poisoned = _run(name)
    np.testing.assert_array_equal(poisoned[0], pred)
    np.testing.assert_array_equal(poisoned[1], full)


def test_dot_product_identity_with_forward_tangents():
    """<w_k, J v_j> from forward_tangents against <J^T w_k, v_j> from the adjoint: the two GPU passes agree."""
    desc, dims, plan, graphs, prm, w = _inputs("qsize")
    v = tj._inputs("qsize")[5]
    eng, b = ts._open(desc, dims, graphs, prm)
    jv = b.forward_tangents(v)[1].astype(np.float64).reshape(len(w), -1)
    jtw = _flat(plan, b.backward_cotangents(w)[1])
    b.close()
    eng.close()
    lhs, rhs = w.astype(np.float64) @ jv.T, jtw @ _flat(plan, v).T
    scale = np.outer(np.linalg.norm(w.astype(np.float64), axis=1), np.linalg.norm(jv, axis=1))
    print("qsize: worst |<w, Jv> - <J^T w, v>| / (|w| |Jv|) %.3g" % (np.abs(lhs - rhs) / scale).max())
    assert np.all(np.abs(lhs - rhs) <= 1e-4 * scale)


@pytest.mark.parametrize("what", ["attention", "convolution", "concat on axis 2", "message network", "readout operation",
                                  "LayerNormalization", "reset_after = false", "128/128", "halo rows", "training step"])
def test_refused_by_name(what):
    _, desc, dims, graphs, prm, kw = next(r for r in tj._refusals() if r[0] == what)
    eng = Engine(MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)), 0)
    eng.set_params(prm)
    b = Batch(eng, graphs, **kw)
    if what == "training step":
        b.enable_training()
        b.forward_train()
    before = None if kw else b.forward().copy()   # (a batch with halo rows forwards in steps, with its neighbours)
    with pytest.raises(EngineError, match="backward jacobian: .*" + what) as e:
        b.backward_cotangents(np.ones((2, b.predictions, b.output_units), np.float32))
    assert e.value.code == -2
    if before is not None:
        np.testing.assert_array_equal(b.forward(), before)
    b.close()
    eng.close()


def test_argument_errors():
    desc, dims, plan, graphs, prm, w = _inputs("s17")
    bare = copy.deepcopy(desc)   # the same model, its links without features
    bare["entities"][[e["name"] for e in bare["entities"]].index("link")]["features"] = []
    bare_plan = MPPlan.from_model_info(Model_information(copy.deepcopy(bare), dims))
    eng, b = ts._open(bare, dims, graphs, bare_plan.init_params(ts.sc.SEED, bias_scale=ts.sc.BIAS))
    for bad in (w[0], w[:, :-1], np.zeros((0,) + w.shape[1:], np.float32)):
        with pytest.raises(ValueError, match="backward_cotangents: .*shape"):
            b.backward_cotangents(bad)
    assert sorted(b.backward_cotangents(w)[1]) == ["path"]
    E, cot = len(bare_plan.entities), np.ascontiguousarray(w[:2, :, None])
    bufs = [np.zeros((2, r, 4), np.float32) for r in b.rows]
    only_path = (C.c_void_p * E)(*[a.ctypes.data if fs else None for a, fs in zip(bufs, bare_plan.features)])
    every = (C.c_void_p * E)(*[a.ctypes.data for a in bufs])
    for n_cot, c, n_ents, outs in [(0, cot.ctypes.data, E, only_path), (2, None, E, only_path), (2, cot.ctypes.data, E, None),
                                   (2, cot.ctypes.data, E + 1, only_path), (2, cot.ctypes.data, E, every)]:
        assert lib.ign_backward_jacobian(b.handle, n_cot, c, n_ents, None, outs) == -1
    assert lib.ign_backward_jacobian(b.handle, 2, cot.ctypes.data, E, None, only_path) == 0
    b.close()
    eng.close()


def test_model_level_call_follows_sensitivities(monkeypatch):
    desc, dims, plan, graphs, prm, w = _inputs("s17")
    desc = copy.deepcopy(desc)
    for e in desc["entities"]:
        for f in e["features"]:
            if f["name"] == "traffic":
                f["normalization"] = "halve"
    monkeypatch.setitem(generate_model.user_namespace, "halve", lambda x, name: x * np.float32(0.5))
    model = ComnetModel(Model_information(desc, dims), params=prm)
    pred, rows = model.jacobian_rows(graphs, cotangents=w[:3])
    b = model.batch(graphs)   # (the model's batch: built from the halved values)
    want = b.backward_cotangents(w[:3])
    b.close()
    _same_bits((pred, {"rows": _flat(plan, rows)}), (want[0], {"rows": _flat(plan, want[1])}), "jacobian_rows against Batch.backward_cotangents")
    sens = model.sensitivities(graphs, dpred=np.array(w[1]))
    assert _rel(_flat(plan, rows)[1], _flat(plan, {e: {f: a[None] for f, a in fs.items()} for e, fs in sens[1].items()})[0]) <= 1e-4
    picked, one_hot = model.jacobian_rows(graphs, predictions=[16, 0]), model.jacobian_rows(graphs, cotangents=np.eye(len(w[0]), dtype=np.float32)[[16, 0]])
    np.testing.assert_array_equal(_flat(plan, picked[1]), _flat(plan, one_hot[1]), err_msg="predictions= against one-hot cotangents")
    with pytest.raises(ValueError, match="jacobian_rows"):
        model.jacobian_rows(graphs)
    model.engine.close()
