"""The table of tests/aggregation_cases.py on the GPU: the attention, convolution and concat MPs on graphs
whose attention groups, in-degrees and destination rows sit on their kernels' edges (the 64-lane cell
stride, the four-group block, groups with empty cells, with one cell and with none, two messages in one
cell, logits where exp overflows, in-degrees 0 / 1 / 3 / 4 / 5 / 64, 15 / 16 / 17 rows), at H = 16 / 32
(concat: 64 too), T = 2.

Every bound is an existing one: test_gpu_parity's _close (1e-4 max(1, |y|) against the float64 oracle) for
predictions and final states, test_gpu_training's _check_grads (GTOL per tensor, loss and l2 at 1e-5)
against float64 autograd.  Everything else is bitwise: a graph alone and in its batch, uncached and
NaN-poisoned pool blocks, a second run, the JSON-lowered plan."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from ignnition_amd import _lib
from ignnition_amd.engine import Batch, Engine, device_count
from tests import aggregation_cases as ac
from tests.test_gpu_parity import TOL, _close, _scaled_err
from tests.test_gpu_training import GTOL, _check_grads

pytestmark = pytest.mark.gpu

ALL = sorted(ac.CASES)
WITH_STATES = ac.ATTENTION + ac.CONVOLUTION
POOLED = ["att_l65", "qatt_p17", "conv_deg5"]       # attention with empties, two-source attention, convolution
JSON = ["att_l65", "conv_l17", "cat2_p17"]
TWICE = ["att_l129", "att_dup", "qatt_p65", "conv_deg64", "conv_idle", "cat1_long"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _run(name, graphs=None, json_plan=False, train=True):
    """One fresh engine under the current environment: the inference forward's predictions and final
    states, then the training forward's predictions, the loss and the flat gradient of one backward."""
    desc, dims, _, plan, g, labels, prm = ac.case_inputs(name)
    if graphs is None:
        graphs = g
    else:
        labels = [labels[[id(x) for x in g].index(id(y))] for y in graphs]
    eng = Engine(plan, 0)
    if json_plan:
        h = C.c_void_p()
        _lib.check(_lib.lib.ign_plan_create_json(json.dumps(desc).encode(), json.dumps(dims).encode(), 0, C.byref(h)))
        _lib.lib.ign_plan_destroy(eng.handle)
        eng.handle = h
    eng.set_params(prm)
    b = Batch(eng, graphs)
    try:
        r = {"out": b.forward().reshape(-1).copy(), "states": {e: b.state(e) for e in plan.entities}}
        if train:
            b.enable_training()
            r["pred"] = b.forward_train().reshape(-1).copy()
            y = torch.tensor(np.concatenate([np.asarray(l, np.float32).reshape(-1) for l in labels]), device="cuda")
            dpred = torch.empty_like(y)
            r["loss"] = eng.mse_loss(b.predictions_ptr(), y, dpred)
            grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
            b.backward(dpred, grads)
            torch.cuda.synchronize()
            r["grads"] = grads.cpu().numpy()
            r["named"] = {n: r["grads"][off:off + int(np.prod(shape))].reshape(shape) for n, shape, off in eng.layout}
        return r
    finally:
        b.close()
        eng.close()


_BASE = {}


def _base(name):
    """The default environment's run, once per case, shared by the bitwise tests (read-only)."""
    if name not in _BASE:
        _BASE[name] = _run(name)
    return _BASE[name]


def _same_bits(got, exp, what, keys=("out", "pred", "grads")):
    for k in keys:
        np.testing.assert_array_equal(got[k], exp[k], err_msg="%s: %s" % (what, k))
    for e in exp["states"]:
        np.testing.assert_array_equal(got["states"][e], exp["states"][e], err_msg="%s: final %s states" % (what, e))


def _close_where_finite(got, ref, what):
    """NaN exactly where the oracle's is, _close everywhere else."""
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what + ": NaN pattern")
    _close(got[~nan], ref[~nan])


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in ALL if n != "logit_overflow"])
def test_forward_matches_oracle(name):
    """Predictions (the inference and the training forward) and, for attention and convolution, every
    entity's final state against DenseOracle; in the degree-0 cases the idle link's state is NaN exactly
    where the oracle's is."""
    ref, ref_states, _ = ac.reference(name)
    r = _base(name)
    errs = {"predictions": _scaled_err(r["out"], ref)}
    _close(r["out"], ref)
    _close(r["pred"], ref)
    if name in WITH_STATES:
        for e, s in r["states"].items():
            assert s.shape == ref_states[e].shape, e
            _close_where_finite(s, ref_states[e], "%s %s" % (name, e))
            errs[e] = _scaled_err(s[~np.isnan(s)], ref_states[e][~np.isnan(ref_states[e])])
    if ac.CASES[name].idle is not None:
        assert np.isnan(r["states"]["link"][ac.CASES[name].idle]).all()
    print("%s: max scaled error vs float64 oracle %s" % (name, {k: "%.3g" % v for k, v in errs.items()}))


def test_logit_overflow():
    """Scores up to about +3e3 and down to about -3e2, empty cells in two groups, one-cell groups below -90: exp(e) alone is inf in float32,
    the empty cells' exp(-mx) is 0.  Predictions and final states finite and within the larger of _close's
    TOL and 4x the float32 DenseOracle's own worst error against float64 (__expf's 1-2 ulp against libm
    over T = 2 iterations).

    Measured on an MI355X: the float32 oracle's worst scaled error is 3.45e-7, so the bound is TOL; the
    engine lies within it.  (Before attn_softmax_kernel stopped adding 0 * exp(-mx) for groups without an
    empty cell, the engine's error was 2.97: the one-cell groups' weights were NaN.)"""
    ref, ref_states, _ = ac.reference("logit_overflow")
    f32 = ac.reference("logit_overflow", np.float32)[0]
    r = _run("logit_overflow", train=False)
    yard, err = _scaled_err(f32, ref), _scaled_err(r["out"], ref)
    tol = max(TOL, 4.0 * yard)
    print("logit_overflow: float32 oracle max scaled error %.3g, engine %.3g, tolerance %.3g" % (yard, err, tol))
    assert np.isfinite(r["out"]).all()
    _close(r["out"], ref, tol)
    for e, s in r["states"].items():
        _close(s, ref_states[e], tol)


@pytest.mark.parametrize("name", ac.GRADS)
def test_gradients(name):
    desc, dims, _, _, graphs, labels, prm = ac.case_inputs(name)
    print(name)
    eng, b, grads = _check_grads(desc, dims, graphs, labels, prm, oracle=ac.grad_reference(name))
    g = grads.cpu().numpy()
    b.close()
    eng.close()
    assert np.isfinite(g).all() and np.abs(g).sum() > 0


@pytest.mark.parametrize("name", ac.DEG0)
def test_gradients_with_an_idle_destination(name):
    """Degree 0: autograd carries the idle link's 0 / 0 into the tensors of the link's update cell and
    into no other.  The engine's gradient holds non-finite entries in the same tensors; every finite
    tensor is within GTOL, the loss within 1e-5.

    Two tensors failed this before their fixes, both by NaN * 0 on the idle row: convolution/kernel
    (conv_bwd_kernel now writes a zero du row for a destination without a message) and path_update/kernel
    (the link -> path update's weight gradient contracts every link row with its table gradient; in a plan
    with a convolution MP the rows that no step reads now enter that contraction as zeros)."""
    o_loss, _, o_g, o_pred = ac.grad_reference(name)
    r = _base(name)
    np.testing.assert_allclose(r["pred"], o_pred, rtol=1e-4, atol=1e-4)
    assert r["loss"] == pytest.approx(o_loss, rel=1e-5)
    bad = sorted(n for n, g in o_g.items() if not np.isfinite(g).all())
    assert sorted(n for n, g in r["named"].items() if not np.isfinite(g).all()) == bad
    assert 0 < len(bad) < len(o_g)
    for n, og in o_g.items():
        if n not in bad:
            err = np.linalg.norm(r["named"][n].astype(np.float64) - og)
            assert err <= GTOL * np.linalg.norm(og) + 1e-7, "%s: rel err %.3g" % (n, err / max(np.linalg.norm(og), 1e-30))


@pytest.mark.parametrize("name", ac.BATCHES)
def test_batch_equals_graph_alone(name):
    """Groups are per graph and a destination's messages keep their order: each graph's predictions and
    final states in the batch are bitwise those of the graph in a batch of its own."""
    graphs = ac.case_inputs(name)[4]
    base = _base(name)
    parts = [_run(name, [g], train=False) for g in graphs]
    got = {"out": np.concatenate([p["out"] for p in parts]),
           "states": {e: np.concatenate([p["states"][e] for p in parts], axis=0) for e in base["states"]}}
    _same_bits(got, base, "graph by graph", keys=("out",))


@pytest.mark.parametrize("env", [{"IGN_POOL": "0"}, {"IGN_POOL": "1", "IGN_POOL_POISON": "1"}], ids=["uncached", "poisoned"])
@pytest.mark.parametrize("name", POOLED)
def test_pool_blocks_do_not_change_the_bits(monkeypatch, name, env):
    """ecell, msg_w, dw, dv, ds and sum_save are pooled: uncached blocks, and cached blocks that start as
    NaN, give the bits of the default run in forward, forward_train and backward (no kernel reads an
    element that a group's early return or a c == 0 store left unwritten)."""
    base = _base(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _same_bits(_run(name), base, " ".join("%s=%s" % kv for kv in env.items()))


@pytest.mark.parametrize("name", TWICE)
def test_two_runs_give_the_same_bits(name):
    """The backward has no atomics: a second engine gives the same gradient bits (NaN bits included)."""
    base, again = _base(name), _run(name)
    _same_bits(again, base, "second run", keys=("out", "pred"))
    np.testing.assert_array_equal(again["grads"].view(np.uint32), base["grads"].view(np.uint32))


@pytest.mark.parametrize("name", JSON)
def test_json_plan_gives_the_same_bits(name):
    _same_bits(_run(name, json_plan=True), _base(name), "ign_plan_create_json")
