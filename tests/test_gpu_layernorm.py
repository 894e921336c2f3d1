"""LayerNormalization layers in the readout's Dense stacks on the GPU (layernorm_kernels.hip,
dense_stack.cpp, the inference readout): NSFNET samples, H = 32, 3 iterations
(tests/layernorm_cases.py, tests/predict_cases.py).

ign_forward and the training forward follow the float64 oracle at the widths where the kernels
change their row layout (test_gpu_dropout's prediction tolerance); a row of equal values reads
exactly beta; gradients, gamma's and beta's included, and Adam steps follow float64 autograd
(test_gpu_training's GTOL per gradient tensor, test_gpu_train_steps' rule for the updated
parameters); two runs, and poisoned or uncached pool blocks, give the same bits; a model without the
layer keeps the fused readout."""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch

from ignnition_amd import _lib
from ignnition_amd.engine import Batch, Engine, MPPlan, device_count
from ignnition_amd.json_operations import Model_information
from ignnition_amd.training import Trainer, host_loss
from oracle.train_oracle import adam_step
from tests import layernorm_cases as lc
from tests.predict_cases import layer_name, predict_model
from tests.test_gpu_training import GTOL

pytestmark = pytest.mark.gpu

SEED, STEP = 0x5DEECE66D1234567, 3
LN_GAMMA, LN_BETA = "readout_model_0/ln/gamma", "readout_model_0/ln/beta"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _engine(desc, dims, prm):
    eng = Engine(MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)), 0)
    eng.set_params(prm)
    return eng


def _forwards(desc, dims, graphs, prm):
    """(ign_forward twice, the training forward) of a fresh engine."""
    eng = _engine(desc, dims, prm)
    b = Batch(eng, graphs)
    try:
        first = b.forward().copy()
        again = b.forward().copy()   # (the captured replay)
        b.enable_training()
        return first, again, b.forward_train().copy()
    finally:
        b.close()
        eng.close()


def _train(desc, dims, graphs, labels, prm, stream=(SEED, STEP)):
    """One training forward and backward on a fresh engine: (predictions, flat gradient, {name: gradient})."""
    eng = _engine(desc, dims, prm)
    b = Batch(eng, graphs)
    try:
        b.enable_training()
        b.set_dropout(*stream)
        pred = b.forward_train().copy()
        y = torch.tensor(np.concatenate([np.asarray(l, np.float32).reshape(-1) for l in labels]), device="cuda")
        dpred = torch.empty_like(y)
        eng.mse_loss(b.predictions_ptr(), y, dpred)
        grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
        b.backward(dpred, grads)
        torch.cuda.synchronize()
        g = grads.cpu().numpy()
        return pred, g, {name: g[off:off + int(np.prod(shape))].reshape(shape) for name, shape, off in eng.layout}
    finally:
        b.close()
        eng.close()


def _assert_grads(named, o_g, what=""):
    rel = {n: np.linalg.norm(named[n].astype(np.float64) - og) / max(np.linalg.norm(og), 1e-30) for n, og in o_g.items()}
    worst = max(rel, key=rel.get)
    print("%sworst gradient tensor vs float64 autograd: %s, relative L2 %.3g" % (what, worst, rel[worst]))
    for n, og in o_g.items():
        err = np.linalg.norm(named[n].astype(np.float64) - og)
        assert err <= GTOL * np.linalg.norm(og) + 1e-7, "%s%s: rel err %.3g" % (what, n, rel[n])


def _check_forward(desc, n_graphs=2):
    dims, plan, graphs, _, prm = lc.inputs(desc, n_graphs=n_graphs)
    ref = lc.make_oracle(desc, dims, prm, plan, graphs).forward(graphs).detach().numpy().reshape(-1)
    first, again, train = _forwards(desc, dims, graphs, prm)
    assert np.isfinite(ref).all()
    print("max |ign_forward - oracle| %.3g, max |forward_train - oracle| %.3g, oracle range %.3g"
          % (np.abs(first.reshape(-1) - ref).max(), np.abs(train.reshape(-1) - ref).max(), np.ptp(ref)))
    np.testing.assert_array_equal(first, again)
    np.testing.assert_allclose(first.reshape(-1), ref, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(train.reshape(-1), ref, rtol=1e-4, atol=1e-4)
    return prm, ref, first, train


WIDTHS = [1, 7, 16, 24, 64, 256, 300]


@pytest.mark.parametrize("units", WIDTHS)
def test_forward_at_each_row_layout(units):
    """Dense(units, tanh), LayerNormalization, Dense(1) on 364 path rows: 16 / 32 / 64 lanes per row, the
    float4 and the strided four-per-lane rows, and the looping wide row."""
    _, ref, _, _ = _check_forward(lc.width_model(units))
    assert ref.size == 364 and (units == 1 or np.ptp(ref) > 1e-2)


@pytest.mark.parametrize("units", WIDTHS)
def test_forward_of_a_last_layer(units):
    """The layer after the last Dense layer: the predictions [364][units] are its output.  At width 1 a
    row centres to zero, so every prediction is exactly beta."""
    prm, ref, first, train = _check_forward(lc.last_model(units))
    assert first.size == 364 * units
    if units == 1:
        assert (first == prm["readout_model_0/ln/beta"][0]).all() and (train == prm["readout_model_0/ln/beta"][0]).all()
    else:
        assert np.ptp(ref) > 1e-2


@pytest.mark.parametrize("n_graphs", [2, 3])
def test_forward_on_pooled_graph_rows(n_graphs):
    """Predict on one row per graph, a width-16 layer first: 2 or 3 rows, fewer than the 4 rows one wave
    holds at that width; a width-24 layer inside the readout operation in front of the pooling."""
    _, ref, first, _ = _check_forward(lc.pooled_model(), n_graphs)
    assert first.size == n_graphs and np.ptp(ref) > 1e-3


def test_degenerate_rows_read_beta():
    """A relu layer whose bias is -1e3 writes zero rows: the layer in ign_forward and in the training
    forward reads exactly beta on every row, and every gradient through it is finite."""
    desc = lc.degenerate_model(last=True)
    dims, plan, graphs, _, prm = lc.inputs(desc)
    prm = dict(prm)
    prm["readout_model_0/%s/bias" % layer_name(0)] = np.full(16, -1e3, np.float32)
    first, again, train = _forwards(desc, dims, graphs, prm)
    beta = np.broadcast_to(prm[LN_BETA], (364, 16))
    assert np.ptp(prm[LN_BETA]) > 0
    np.testing.assert_array_equal(first.reshape(364, 16), beta)
    np.testing.assert_array_equal(train.reshape(364, 16), beta)
    desc = lc.degenerate_model(last=False)
    dims, plan, graphs, labels, prm = lc.inputs(desc)
    prm = dict(prm)
    prm["readout_model_0/%s/bias" % layer_name(0)] = np.full(16, -1e3, np.float32)
    pred, g, named = _train(desc, dims, graphs, labels, prm)
    assert np.isfinite(pred).all() and np.ptp(pred) == 0
    assert np.isfinite(g).all()
    assert np.abs(named[LN_BETA]).sum() > 0
    _, _, o_g, o_pred = lc.make_oracle(desc, dims, prm, plan, graphs).loss_and_grads(graphs, labels)
    np.testing.assert_allclose(pred.reshape(-1), o_pred, rtol=1e-4, atol=1e-4)
    _assert_grads(named, o_g)


_RUNS = {}


def _grad_case(case):
    if case not in _RUNS:
        desc = lc.GRAD_CASES[case]()
        dims, plan, graphs, labels, prm = lc.inputs(desc)
        _RUNS[case] = (desc, dims, plan, graphs, labels, prm, _train(desc, dims, graphs, labels, prm))
    return _RUNS[case]


@pytest.mark.parametrize("case", sorted(lc.GRAD_CASES))
def test_gradients_match_autograd(case):
    desc, dims, plan, graphs, labels, prm, (pred, _, named) = _grad_case(case)
    ora = lc.make_oracle(desc, dims, prm, plan, graphs, SEED, STEP)
    _, _, o_g, o_pred = ora.loss_and_grads(graphs, labels)
    assert set(o_g) == set(prm) == set(named)
    assert sum(n.endswith("/gamma") or n.endswith("/beta") for n in o_g) == sum(s[5] + s[6] for s in plan.layernorm_sites())
    assert len(plan.layernorm_sites()) >= 1
    if case.startswith("no_affine"):
        # the tolerances assume the normalisation amplifies upstream rounding by no more than
        # 1 / sqrt(epsilon) of the default epsilon: with epsilon 1e-5 the rows' own variance must do it.
        # A condition on the inputs (the float64 oracle alone)
        print("smallest row variance entering the epsilon 1e-5 layer: %.3g" % min(ora.min_var.values()))
        assert len(ora.min_var) == 1 and min(ora.min_var.values()) >= 1e-3
    if case != "odd_widths_first_last":   # (a last layer of width 1 passes no gradient below it)
        assert np.ptp(o_pred) > 1e-3
        for n, og in o_g.items():
            assert np.linalg.norm(og) > 0, n
    else:
        assert np.linalg.norm(o_g["readout_model_0/layer_4_LayerNormalization_readout/beta"]) > 0
    np.testing.assert_allclose(pred.reshape(-1), o_pred, rtol=1e-4, atol=1e-4)
    _assert_grads(named, o_g)


def test_two_runs_give_the_same_bits():
    desc, dims, plan, graphs, labels, prm, (pred, g, _) = _grad_case("with_dropout")
    p1, g1, _ = _train(desc, dims, graphs, labels, prm)
    np.testing.assert_array_equal(p1, pred)
    np.testing.assert_array_equal(g1, g)


@pytest.mark.parametrize("env", [{"IGN_POOL": "0"}, {"IGN_POOL": "1", "IGN_POOL_POISON": "1"}], ids=["uncached", "poisoned"])
def test_pool_blocks_do_not_change_the_bits(monkeypatch, env):
    """The layers' buffers, statistics and partial sums come from the device pool: uncached blocks, and
    cached blocks that start as NaN, give the predictions and gradients of the default run."""
    desc, dims, plan, graphs, labels, prm, (pred, g, _) = _grad_case("four_layer")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p1, g1, _ = _train(desc, dims, graphs, labels, prm)
    np.testing.assert_array_equal(p1, pred)
    np.testing.assert_array_equal(g1, g)
    eng = _engine(desc, dims, prm)
    b = Batch(eng, graphs)
    try:
        np.testing.assert_allclose(b.forward().reshape(-1), pred.reshape(-1), rtol=1e-4, atol=1e-4)
    finally:
        b.close()
        eng.close()


def test_trainer_steps_move_gamma_and_beta():
    """Three Trainer.train_step with Adam on the four_layer case, the same batch each step: the gradient
    of step k against float64 autograd at the parameters the step started from (GTOL per tensor), the
    updated parameters against the float64 Keras Adam fed the engine's gradient (rtol 1e-5 / atol 1e-6,
    test_gpu_train_steps' rule); every tensor moves, gamma and beta too; Trainer.evaluate is the
    inference forward."""
    desc = lc.GRAD_CASES["four_layer"]()
    dims, plan, graphs, labels, prm = lc.inputs(desc)
    mi = Model_information(copy.deepcopy(desc), dims)
    tr = Trainer(mi, params=prm, seed=11)
    eng = tr.engine
    try:
        flat = lambda t: {name: t[off:off + int(np.prod(shape))].reshape(shape).astype(np.float64)
                          for name, shape, off in eng.layout}
        assert sum(n.endswith("/gamma") or n.endswith("/beta") for n in prm) == 4
        for k in range(3):
            p_k = tr.params()
            ref = {n: x.astype(np.float64) for n, x in p_k.items()}
            rm, rv = flat(tr.m.cpu().numpy()), flat(tr.v.cpu().numpy())
            out = tr.train_step(graphs, labels)
            g = tr.grads.cpu().numpy()
            named = {name: g[off:off + int(np.prod(shape))].reshape(shape) for name, shape, off in eng.layout}
            o_loss, _, o_g, _ = lc.make_oracle(desc, dims, p_k, plan, graphs, 11, k).loss_and_grads(graphs, labels)
            assert out["loss"] == pytest.approx(o_loss, rel=1e-5)
            _assert_grads(named, o_g, "step %d: " % k)
            lr, b1, b2, eps = (float(np.float32(h)) for h in (out["learning_rate"], 0.9, 0.999, 1e-7))
            adam_step(ref, {n: named[n].astype(np.float64) for n in ref}, rm, rv, k, lr, b1, b2, eps)
            got = tr.params()
            for n in ref:
                assert not np.array_equal(got[n], p_k[n]), n
                np.testing.assert_allclose(got[n], ref[n], rtol=1e-5, atol=1e-6, err_msg="step %d, %s" % (k, n))
        b = tr.model.batch(graphs)
        try:
            p = b.forward().reshape(-1).astype(np.float64)
        finally:
            b.close()
        o_p = lc.make_oracle(desc, dims, tr.params(), plan, graphs).forward(graphs).detach().numpy().reshape(-1)
        np.testing.assert_allclose(p, o_p, rtol=1e-4, atol=1e-4)
        y = np.concatenate([np.asarray(l, np.float64).reshape(-1) for l in labels])
        ev = tr.evaluate([(graphs, labels)])
        assert ev["loss"] == host_loss(tr.loss_kind, p, y)
        assert ev["prediction/mean"] == float(np.asarray(tr._denorm(p), np.float64).mean())
    finally:
        eng.close()


def test_split_batch_runs_the_layer():
    """SplitBatch sub-plans (the engine's replicas) carry the layer: the split forward equals the whole one."""
    from ignnition_amd.engine import SplitBatch
    desc = lc.GRAD_CASES["four_layer"]()
    dims, plan, graphs, _, prm = lc.inputs(desc, n_graphs=4)
    eng = _engine(desc, dims, prm)
    try:
        b = Batch(eng, graphs)
        whole = b.forward().copy()
        b.close()
        sb = SplitBatch(eng, graphs, 2)
        try:
            np.testing.assert_array_equal(sb.forward(), whole)
        finally:
            sb.close()
    finally:
        eng.close()


def test_a_model_without_the_layer_keeps_the_fused_readout():
    """The selu 256-256-1 readout without a LayerNormalization: one readout launch (the fused kernel), the
    bits of a second engine built from the same description, and ign_plan_describe_json's parameter
    list as the plan names it; with the layer between its Dense layers the stack runs layer by layer."""
    desc = predict_model("selu")
    dims, plan, graphs, _, prm = lc.inputs(desc)
    outs = []
    for _ in range(2):
        eng = _engine(desc, dims, prm)
        b = Batch(eng, graphs)
        try:
            eng.set_timing(True)
            outs.append(b.forward().copy())
            assert eng.stats()["readout"]["launches"] == 1
        finally:
            b.close()
            eng.close()
    np.testing.assert_array_equal(outs[0], outs[1])
    h = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create_json(json.dumps(desc).encode(), json.dumps(dims).encode(), 0, C.byref(h)))
    try:
        need = C.c_int64()
        _lib.check(_lib.lib.ign_plan_describe_json(h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        _lib.check(_lib.lib.ign_plan_describe_json(h, buf, need.value, C.byref(need)))
        doc = json.loads(buf.value.decode())
    finally:
        _lib.lib.ign_plan_destroy(h)
    assert [(p["name"], tuple(p["shape"])) for p in doc["params"]] == [(n, tuple(s)) for n, s in plan.param_specs()]
    assert len(doc["params"]) == 12 and doc["layernorm"] == []
    with_ln = lc.ln_model("selu", [(1, lc.ln())])
    dims, plan2, graphs, _, prm2 = lc.inputs(with_ln)
    eng = _engine(with_ln, dims, prm2)
    b = Batch(eng, graphs)
    try:
        eng.set_timing(True)
        out = b.forward().copy()
        assert eng.stats()["readout"]["launches"] == 4   # three Dense layers and the LayerNormalization
    finally:
        b.close()
        eng.close()
    ref = lc.make_oracle(with_ln, dims, prm2, plan2, graphs).forward(graphs).detach().numpy().reshape(-1)
    np.testing.assert_allclose(out.reshape(-1), ref, rtol=1e-4, atol=1e-4)
