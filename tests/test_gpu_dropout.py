"""Dropout layers in the readout's Dense stacks on the GPU (dropout_kernels.hip, train.cpp): NSFNET
samples, H = 32, 3 iterations (tests/dropout_cases.py, tests/predict_cases.py).

Inference is the identity (the fused readout stays); rate 0 is no layer; the device mask is
ign_dropout_keep's, bit for bit; gradients and Adam steps follow float64 autograd with the same masks
(tolerances: test_gpu_training's GTOL per gradient tensor and its prediction tolerance,
test_gpu_train_steps' for the updated parameters); a dropped inf reads 0; poisoned or uncached pool
blocks give the same bits."""
import copy

import numpy as np
import pytest
import torch

from ignnition_amd import _lib
from ignnition_amd.engine import Batch, Engine, MPPlan, device_count, dropout_keep
from ignnition_amd.json_operations import Model_information
from ignnition_amd.training import Trainer, host_loss
from oracle.train_oracle import adam_step
from tests import dropout_cases as dc
from tests.predict_cases import layer_name, predict_model
from tests.test_gpu_training import GTOL

pytestmark = pytest.mark.gpu

SEED, STEP = 0x5DEECE66D1234567, 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _engine(desc, dims, prm):
    eng = Engine(MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)), 0)
    eng.set_params(prm)
    return eng


def _train(desc, dims, graphs, labels, prm, stream=None):
    """One training forward and backward on a fresh engine: (predictions, flat gradient, {name: gradient})."""
    eng = _engine(desc, dims, prm)
    b = Batch(eng, graphs)
    try:
        b.enable_training()
        if stream is not None:
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


@pytest.mark.parametrize("case", ["selu", "odd_widths"])
def test_inference_is_identity(case):
    """ign_forward of the description with Dropout(0.5) after layer 0 is bitwise that of the description
    without it (selu: both on the fused readout kernels), and the site list is closed once a batch exists."""
    plain = predict_model(case)
    dims, plan, graphs, _, prm = dc.inputs(plain)
    outs = []
    for desc in (plain, dc.insert_dropout(plain, [(1, 0.5, {})])):
        eng = _engine(desc, dims, prm)
        b = Batch(eng, graphs)
        try:
            outs.append(b.forward().copy())
            assert _lib.lib.ign_plan_add_dropout(eng.handle, -1, 1, 0.5, 0) == -1
        finally:
            b.close()
            eng.close()
    assert np.isfinite(outs[0]).all() and np.ptp(outs[0]) > 0
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.parametrize("case", ["selu", "four_layer"])
def test_rate_zero_is_no_layer(case):
    plain = predict_model(case)
    dims, plan, graphs, labels, prm = dc.inputs(plain)
    p0, g0, _ = _train(plain, dims, graphs, labels, prm)
    p1, g1, _ = _train(dc.insert_dropout(plain, [(1, 0.0, {}), (len(plan.dense), 0.0, {})]), dims, graphs, labels, prm,
                       stream=(SEED, STEP))
    assert np.abs(g0).sum() > 0
    np.testing.assert_array_equal(p0, p1)
    np.testing.assert_array_equal(g0, g1)


def _mask_model(rate):
    """One Dense layer of 7 linear units, then a Dropout (rate None: no such layer): the predictions are the
    masked layer output."""
    desc = predict_model("one_layer")
    for net in desc["neural_networks"]:
        if net["nn_name"] == "readout_model":
            net["nn_architecture"] = [{"type_layer": "Dense", "name": layer_name(0), "units": 7, "activation": "None"},
                                      {"type_layer": "Dropout", "rate": rate}][:2 if rate is not None else 1]
    return desc


def _forward_train(desc, dims, graphs, prm, streams):
    eng = _engine(desc, dims, prm)
    b = Batch(eng, graphs)
    try:
        b.enable_training()
        out = []
        for s in streams:
            if s is not None:
                b.set_dropout(*s)
            out.append(b.forward_train().copy())
        return out
    finally:
        b.close()
        eng.close()


def test_device_mask_is_the_host_function():
    """364 x 7 = 2548 predictions: zero exactly where ign_dropout_keep drops, elsewhere bitwise
    float32(y) * float32(1 / (1 - rate)) with y the rate-0 forward.  A batch whose stream was never set
    draws (0, 0); another step draws another mask; the same (seed, step) gives the same bits."""
    rate = 0.25
    dims, plan, graphs, _, prm = dc.inputs(_mask_model(rate))
    (y,) = _forward_train(_mask_model(0.0), dims, graphs, prm, [None])
    assert y.shape == (364, 7) and np.isfinite(y).all()
    z00, z1, z2, z1b = _forward_train(_mask_model(rate), dims, graphs, prm,
                                      [None, (SEED, STEP), (SEED, STEP + 1), (SEED, STEP)])
    scale = np.float32(1.0 / (1.0 - rate))
    masks = []
    for z, (seed, step) in ((z00, (0, 0)), (z1, (SEED, STEP)), (z2, (SEED, STEP + 1))):
        keep = dropout_keep(seed, 0, step, 364, 7, rate).astype(bool)
        masks.append(keep)
        assert 0.6 < keep.mean() < 0.9
        assert (z[~keep] == 0.0).all()
        np.testing.assert_array_equal(z[keep], (y * scale)[keep])
    assert (masks[1] != masks[2]).any() and (masks[0] != masks[1]).any()
    np.testing.assert_array_equal(z1, z1b)


def test_dropped_non_finite_reads_zero():
    """The output kernel x 1e38 x 8: y overflows before the mask.  A dropped element is selected to 0.0,
    never multiplied by it.  (x 1e38 alone does not overflow here: with glorot kernels of magnitude <= 0.39
    the float64 oracle's largest |y| is 0.5e38 .. 1.4e38 over parameter seeds 0 .. 39, below float32's
    3.4e38.  x 8 more keeps every kernel element finite, <= 3.13e38, and puts 653 of the 2548 oracle outputs
    beyond float32, 149 of them under a dropped element for this mask; the test asserts at least one.)"""
    from oracle.dense_forward import DenseOracle
    rate = 0.25
    desc = _mask_model(rate)
    dims, plan, graphs, _, prm = dc.inputs(desc)
    k = "readout_model_0/" + layer_name(0) + "/kernel"
    big = dict(prm)
    big[k] = prm[k] * np.float32(1e38) * np.float32(8)
    assert np.isfinite(big[k]).all()
    keep = dropout_keep(SEED, 0, STEP, 364, 7, rate).astype(bool)
    y64 = DenseOracle(_mask_model(None), dims, {n: v.astype(np.float64) for n, v in big.items()}).forward(graphs).reshape(364, 7)
    over = np.abs(y64) > 1.01 * float(np.finfo(np.float32).max)   # (a margin for the float32 sum's own rounding)
    print("float64 oracle: %d of %d outputs beyond float32, %d of them dropped" % (over.sum(), over.size, (over & ~keep).sum()))
    assert (over & ~keep).sum() >= 1
    (y,) = _forward_train(_mask_model(0.0), dims, graphs, big, [None])
    assert not np.isfinite(y[over]).any()
    (z,) = _forward_train(desc, dims, graphs, big, [(SEED, STEP)])
    assert (z[~keep] == 0.0).all() and not np.isnan(z[~keep]).any()
    assert not np.isfinite(z[keep & over]).any()


GRAD_CASES = {
    "four_layer": lambda: dc.dropout_model("four_layer", [(1, 0.5, {}), (3, 0.5, {})]),
    "odd_widths": lambda: dc.dropout_model("odd_widths", [(0, 0.25, {}), (2, 0.25, {})]),
    "readout_op": dc.readout_op_model,
    "nn_two_inputs_first": dc.nn_two_inputs_first_model,
    "predict_two_inputs_first": dc.predict_two_inputs_first_model,
}
_RUNS = {}


def _grad_case(case):
    if case not in _RUNS:
        desc = GRAD_CASES[case]()
        dims, plan, graphs, labels, prm = dc.inputs(desc)
        _RUNS[case] = (desc, dims, plan, graphs, labels, prm, _train(desc, dims, graphs, labels, prm, stream=(SEED, STEP)))
    return _RUNS[case]


@pytest.mark.parametrize("case", sorted(GRAD_CASES))
def test_gradients_match_autograd_with_the_masks(case):
    desc, dims, plan, graphs, labels, prm, (pred, _, named) = _grad_case(case)
    ora = dc.make_oracle(desc, dims, prm, plan, graphs, SEED, STEP)
    _, _, o_g, o_pred = ora.loss_and_grads(graphs, labels)
    assert np.ptp(o_pred) > 1e-3 and set(o_g) == set(prm)
    for n, og in o_g.items():
        assert np.linalg.norm(og) > 0, n
    np.testing.assert_allclose(pred.reshape(-1), o_pred, rtol=1e-4, atol=1e-4)
    _assert_grads(named, o_g)


@pytest.mark.parametrize("env", [{"IGN_POOL": "0"}, {"IGN_POOL": "1", "IGN_POOL_POISON": "1"}], ids=["uncached", "poisoned"])
def test_pool_blocks_do_not_change_the_bits(monkeypatch, env):
    """The per-site buffers come from the device pool: uncached blocks, and cached blocks that start as
    NaN, give the predictions and gradients of the default run."""
    desc, dims, plan, graphs, labels, prm, (pred, g, _) = _grad_case("four_layer")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p1, g1, _ = _train(desc, dims, graphs, labels, prm, stream=(SEED, STEP))
    np.testing.assert_array_equal(p1, pred)
    np.testing.assert_array_equal(g1, g)


def test_trainer_steps_draw_the_step_mask():
    """Three Trainer.train_step with Adam on the four_layer Dropout model, the same batch each step: step k
    draws the mask of (trainer seed, k).  The gradient of step k against float64 autograd with that mask at
    the parameters the step started from (GTOL per tensor), the updated parameters against the float64
    Keras Adam fed the engine's gradient (rtol 1e-5 / atol 1e-6, test_gpu_train_steps' rule);
    Trainer.evaluate is the inference forward: no mask."""
    desc = GRAD_CASES["four_layer"]()
    dims, plan, graphs, labels, prm = dc.inputs(desc)
    mi = Model_information(copy.deepcopy(desc), dims)
    tr = Trainer(mi, params=prm, seed=11)
    eng = tr.engine
    try:
        assert tr.dropout_seed == 11
        flat = lambda t: {name: t[off:off + int(np.prod(shape))].reshape(shape).astype(np.float64)
                          for name, shape, off in eng.layout}
        for k in range(3):
            p_k = tr.params()
            ref = {n: x.astype(np.float64) for n, x in p_k.items()}
            rm, rv = flat(tr.m.cpu().numpy()), flat(tr.v.cpu().numpy())
            out = tr.train_step(graphs, labels)
            g = tr.grads.cpu().numpy()
            named = {name: g[off:off + int(np.prod(shape))].reshape(shape) for name, shape, off in eng.layout}
            o_loss, _, o_g, _ = dc.make_oracle(desc, dims, p_k, plan, graphs, 11, k).loss_and_grads(graphs, labels)
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
        y = np.concatenate([np.asarray(l, np.float64).reshape(-1) for l in labels])
        ev = tr.evaluate([(graphs, labels)])
        assert ev["loss"] == host_loss(tr.loss_kind, p, y)
        assert ev["prediction/mean"] == float(np.asarray(tr._denorm(p), np.float64).mean())
    finally:
        eng.close()
