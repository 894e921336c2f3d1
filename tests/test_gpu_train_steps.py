"""The training forward and the gradient AFTER a parameter update (tests/step_cases.py).

ign::repack (engine.cpp) rebuilds every packed weight form from d_params after ign_plan_set_params and
after each ign_adam_step; about half of them are read only by the training forward or the backward.  A
pack that repack forgets, or a batch / TrainState that keeps something derived from the weights it was
built under (BatchPrefetcher builds every batch of a real run up to ``depth`` steps before it trains),
would leave every step after the first wrong and every test that sets the parameters once green.

1. test_engine_after_a_step_is_a_fresh_engine: after one Adam step from P0 to P1, the training forward's
   predictions, the loss, the l2 term, every gradient and the inference forward of the stepped engine -- on a
   batch reused across the update, on one built and enable_training()-ed before it, on one built after it -- and of an engine
   whose live plan was handed P1 by set_params (checkpoint restore) are bitwise those of a fresh engine at
   P1 (two fresh engines agree bitwise first).  The step moves every gradient tensor by more than
   10 * GTOL (asserted on the engine's own gradients; the oracle's ratios are in step_cases), so no tensor's
   stale pack fits inside a tolerance.
2. test_trainer_steps_at_their_own_parameters: a short Trainer run on batches prepared before the first
   step, each step's loss, l2 term and gradient against float64 autograd at the parameters it started from,
   its Adam update against the float64 Keras restatement fed the engine's gradient.

Which pack of repack / readout_repack a case reaches (engine.cpp, readout.cpp; cp = the GRU cell, dp = a
predict Dense layer):

  launch_pack_gru (cp.pk_w / pk_u / pk_b)       every case (sum_gru<SAVE>, the backward's gate recompute)
  launch_pack_u_bf16 (cp.pk_ubf)                routenet_h32_f32 (IGN_TRAIN_SEQ_H16=0: the split-bf16 ordered
                                                forward), synthetic_h64 (sum variant 7)
  launch_pack_u_f16 (cp.pk_uh)                  routenet_h32 (resident SAVE forward), routenet_h32_per_mp
                                                (seq_gru_h16<SAVE>), qsize, msgnet_ordered
  launch_pack_w_f16 (cp.pk_wh)                  synthetic_h64 (DIN = H = 64 only; read by the inference forward's sum
                                                variant 8, hence the inference forward in every comparison);
                                                routenet_h16 is the H = 16 cell, which has none of the f16 / bf16 packs
  launch_pack_w_bf16 (cp.pk_wbf)                routenet_h32 (the fused projection), synthetic_h64
  launch_pack_a (cp.pk_wt, cp.pk_ut)            routenet_h32_f32 (IGN_BWD_BF=0: the f32 MFMA backward)
  launch_pack_ut_f16 (cp.pk_uth)                routenet_h32, routenet_h32_per_mp, qsize, rn_l16_p32 (the ordered
                                                backward's dh = du U^T)
  launch_pack_gru per concat slice (pk_slice)   concat2_l16_n32_p32; concat1_ln16_p32 is the axis-1 form beside it
  launch_pack_dense_pad (nn dp.pk_w)            msgnet_sum_l2 (two layers, 64 -> 48 -> 32, l2 on the first: the l2
                                                term of ign_backward_end reads the new weights), msgnet_ordered,
                                                msgnet_edge_params (66 columns padded), attention_over_msgnet
  launch_pack_dense (pk_conv)                   convolution_tanh
  launch_attn_vectors (pk_w12)                  attention, attention_over_msgnet
  launch_pack_readout_h16 (dp.pk_h)             routenet_h32 and every case with the 256-selu-256-selu-1 readout at
                                                H 32 / 64 (readout_h16<SAVE>)
  launch_pack_readout_h32 (dp.pk_h32)           routenet_h32_variant5 (allocated and packed under
                                                IGN_READOUT_VARIANT=5 only: readout_h32<SAVE>)
  launch_pack_dense (dp.pk_w)                   routenet_h32_f32 (dense_fwd_kernel), predict_four_layer (256 -> 32)
  launch_pack_dense_bf16 (dp.pk_bf)             the inference forward of every case with the fused readout
  launch_pack_dense_bf16 (dp.pk_bfn),
  launch_pack_dense_bf16_t (dp.pk_bft)          routenet_h32_f32 run with IGN_TRAIN_DENSE_H16=0 alone (dense_bf / _t)
  launch_pack_dense_f16 (dp.pk_hn, dp.pk_ht)    routenet_h32 (dense_h16_t in the backward), routenet_h16 and
                                                predict_nobias_hidden (dense_h16 forward too), predict_four_layer
  launch_pack_a (dp.pk_wt)                      routenet_h32_f32 (IGN_TRAIN_DENSE_BF=0: row_gemm_t)
  no pack (d_params read directly)              predict_odd_widths (dense_generic, row_gemm_t_generic)
  readout_repack: launch_pack_dense (op pk_w)   readout_nn_pool_product (the ``emb`` network, 64 -> 32)
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

from ignnition_amd import model_examples, synthetic, workloads
from ignnition_amd.engine import Batch, Engine, MPPlan, device_count
from ignnition_amd.json_operations import Model_information
from ignnition_amd.training import Trainer
from oracle.train_oracle import TorchOracle, adam_step, exponential_decay
from tests.step_cases import F32, LR, ORACLE_ANCHORED, STEP_CASES, step_ratios
from tests.test_gpu_training import GTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _labels(labels):
    return torch.tensor(np.concatenate([np.asarray(l, np.float32).reshape(-1) for l in labels]), device="cuda")


def _engine(stack, plan, prm):
    """An engine at ``prm`` on torch's current stream, closed when ``stack`` unwinds.  A plan's own stream is
    non-blocking: torch's fill of a fresh ``grads`` / ``m`` / ``v`` would not be ordered with the engine's
    memset, backward and Adam on the same buffer (Trainer sets the stream for the same reason)."""
    eng = Engine(plan, 0)
    stack.callback(eng.close)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.set_params(prm)
    return eng


def _train_batch(stack, eng, graphs):
    b = Batch(eng, graphs)
    stack.callback(b.close)
    b.enable_training()
    return b


def _run(eng, b, y):
    """One training forward, loss and backward of batch ``b``, then its inference forward: (predictions, loss,
    l2 term, flat gradient as numpy, the gradient on the device, inference predictions)."""
    pred = b.forward_train().reshape(-1).copy()
    dpred = torch.empty_like(y)
    loss = eng.mse_loss(b.predictions_ptr(), y, dpred)
    grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    b.backward(dpred, grads)
    torch.cuda.synchronize()
    return pred, loss, eng.l2_loss(), grads.cpu().numpy(), grads, b.forward().reshape(-1).copy()


def _named(eng, flat):
    return {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, shape, off in eng.layout}


def _same_bits(got, exp, what):
    np.testing.assert_array_equal(got[0], exp[0], err_msg="%s: forward_train predictions" % what)
    assert got[1] == exp[1], "%s: loss %r vs %r" % (what, got[1], exp[1])
    assert got[2] == exp[2], "%s: l2 term %r vs %r" % (what, got[2], exp[2])
    np.testing.assert_array_equal(got[5], exp[5], err_msg="%s: inference forward" % what)
    if not np.array_equal(got[3], exp[3]):
        eng = exp[6]
        g, e = _named(eng, got[3].astype(np.float64)), _named(eng, exp[3].astype(np.float64))
        bad = {n: np.linalg.norm(g[n] - e[n]) / max(np.linalg.norm(e[n]), 1e-30) for n in e if not np.array_equal(g[n], e[n])}
        pytest.fail("%s: gradient tensors differ from the fresh engine's (relative L2): %s"
                    % (what, {n: "%.3g" % v for n, v in bad.items()}))


def _fresh(stack, plan, prm, graphs, y):
    eng = _engine(stack, plan, prm)
    return _run(eng, _train_batch(stack, eng, graphs), y) + (eng,)


def _against_oracle(desc, dims, graphs, labels, prm, got):
    """_check_grads' rule (tests/test_gpu_training.py) on a run that was already made."""
    pred, loss, l2, g, _, _, eng = got
    o_loss, o_reg, o_g, o_pred = TorchOracle(desc, dims, prm).loss_and_grads(graphs, labels)
    np.testing.assert_allclose(pred, o_pred, rtol=1e-4, atol=1e-4)
    assert loss == pytest.approx(o_loss, rel=1e-5)
    assert l2 == pytest.approx(o_reg, rel=1e-5)
    g = _named(eng, g.astype(np.float64))
    rel = {n: np.linalg.norm(g[n] - og) / max(np.linalg.norm(og), 1e-30) for n, og in o_g.items()}
    print("worst gradient tensor at P1 vs float64 autograd: %s, relative L2 %.3g" % max((v, k) for k, v in rel.items())[::-1])
    for n, og in o_g.items():
        assert np.linalg.norm(g[n] - og) <= GTOL * np.linalg.norm(og) + 1e-7, "%s: rel err %.3g" % (n, rel[n])


def _one_step(case, monkeypatch, env, anchored=False):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    desc, dims, graphs, labels, p0 = STEP_CASES[case][0]()
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    y = _labels(labels)
    with contextlib.ExitStack() as stack:   # every engine and batch is closed, whichever assertion fails
        # the stepped engine: two training batches built under P0, one of them not run before the update
        a = _engine(stack, plan, p0)
        b_old, b_early = _train_batch(stack, a, graphs), _train_batch(stack, a, graphs)
        at_p0 = _run(a, b_old, y)
        m, v = torch.zeros_like(at_p0[4]), torch.zeros_like(at_p0[4])
        a.adam_step(at_p0[4], m, v, 0, LR)
        p1 = a.get_params()
        for name in p0:
            assert not np.array_equal(p1[name], np.asarray(p0[name], np.float32)), "%s did not move" % name

        # two fresh engines at P1 agree bitwise: the reference of everything below
        ref = _fresh(stack, plan, p1, graphs, y)
        _same_bits(_fresh(stack, plan, p1, graphs, y), ref, "a second fresh engine at P1")
        if anchored:   # and the fresh engine at the stepped parameters is right
            _against_oracle(desc, dims, graphs, labels, p1, ref)

        # the step moved every gradient tensor by much more than the tolerance gradients are held to
        ratios = step_ratios(_named(a, at_p0[3]), _named(a, ref[3]))
        worst = min(ratios, key=ratios.get)
        print("%s: smallest ||g(P1) - g(P0)|| / ||g(P1)|| %.3g (%s)" % (case, ratios[worst], worst))
        assert ratios[worst] > 10 * GTOL, (worst, ratios[worst])
        assert not np.array_equal(ref[0], at_p0[0])

        _same_bits(_run(a, b_old, y), ref, "the batch reused across the update")
        _same_bits(_run(a, b_early, y), ref, "the batch enabled for training before the update")
        _same_bits(_run(a, _train_batch(stack, a, graphs), y), ref, "a batch built after the update")

        # set_params on a live plan (checkpoint restore): an engine that trained at P0, then given P1
        s = _engine(stack, plan, p0)
        b_s = _train_batch(stack, s, graphs)
        np.testing.assert_array_equal(_run(s, b_s, y)[3], at_p0[3])
        s.set_params(p1)
        _same_bits(_run(s, b_s, y), ref, "set_params on a plan that trained")


@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_engine_after_a_step_is_a_fresh_engine(monkeypatch, case):
    _one_step(case, monkeypatch, STEP_CASES[case][1], anchored=case in ORACLE_ANCHORED)


@pytest.mark.parametrize("switch", sorted(F32))
def test_one_switch_off_after_a_step(monkeypatch, switch):
    """routenet_h32 with one of routenet_h32_f32's switches off at a time: IGN_TRAIN_DENSE_H16=0 alone runs
    dense_bf / dense_bf_t on pk_bfn / pk_bft, IGN_BWD_BF=0 alone the f32 backward behind the split-fp16
    forward, ... (with all five off, the later ones in a kernel's choice are never asked)."""
    _one_step("routenet_h32", monkeypatch, {switch: "0"})


# ---------------------------------------------------------------------------------------------
# a short Trainer run
_SCHEDULE = {"type": "ExponentialDecay", "initial_learning_rate": 0.01, "decay_steps": 2, "decay_rate": 0.5,
             "staircase": "True"}


def _abi_f32(*hyper):
    """ign_adam_step takes the rate, beta_1, beta_2 and epsilon as float (as Keras holds them in the variable's
    dtype): the restatement is fed the values the engine is given, so 1 - beta_2 is 1 - 0.999f in both."""
    return [float(np.float32(h)) for h in hyper]


@pytest.mark.parametrize("kind,steps", [("routenet", 4), ("qsize", 2)])
def test_trainer_steps_at_their_own_parameters(kind, steps):
    """RouteNet / Q-size at H 32 (l2 regularisers 0.1, 0.1, 0.01 on the readout), ExponentialDecay with
    decay_steps 2 and staircase: every batch (two NSFNET graphs each, all different) is made by
    Trainer.prepare before the first step, as BatchPrefetcher does.  Step k, from P_k, m_k, v_k: the reported
    loss and regularisation loss within 1e-5 relative of float64 autograd at P_k; Trainer.grads per tensor
    within GTOL (_check_grads' rule); P_k+1, m, v within rtol 1e-5 / atol 1e-6 of the float64 Keras Adam fed
    the engine's gradient, exponential_decay(k) and the hyper-parameters as the C ABI carries them
    (test_adam_step_matches_keras_restatement's bound); the rate and the step count in the returned dict."""
    qs = kind == "qsize"
    desc = model_examples.qsize(iterations=2) if qs else model_examples.routenet(hidden=32, iterations=3)
    desc["learning_options"]["optimizer"] = {"type": "Adam", "schedule": dict(_SCHEDULE)}
    _, dims, _ = workloads.model(kind)
    mi = Model_information(copy.deepcopy(desc), dims)
    data = [workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", 2 * k + g, qsize=qs) for g in range(2)])
            for k in range(steps)]
    tr = Trainer(mi, params=MPPlan.from_model_info(mi).init_params(7, bias_scale=0.1))
    eng = tr.engine
    prepared = []
    try:
        for graphs, labels in data:
            prepared.append(tr.prepare(graphs, labels))
        rates = []
        for k, (graphs, labels) in enumerate(data):
            p_k = tr.params()
            ref = {n: x.astype(np.float64) for n, x in p_k.items()}
            rm, rv = ({n: x.astype(np.float64) for n, x in _named(eng, t.cpu().numpy()).items()} for t in (tr.m, tr.v))
            out = tr.train_prepared(*prepared[k])
            o_loss, o_reg, o_g, _ = TorchOracle(desc, dims, p_k).loss_and_grads(graphs, labels)
            g = _named(eng, tr.grads.cpu().numpy())
            rel = {n: np.linalg.norm(g[n].astype(np.float64) - og) / max(np.linalg.norm(og), 1e-30) for n, og in o_g.items()}
            worst = max(rel, key=rel.get)
            print("step %d: loss %.9g (oracle %.9g), l2 %.9g (oracle %.9g), worst gradient tensor %s %.3g"
                  % (k, out["loss"], o_loss, out["regularization_loss"], o_reg, worst, rel[worst]))
            assert out["loss"] == pytest.approx(o_loss, rel=1e-5)
            assert out["regularization_loss"] == pytest.approx(o_reg, rel=1e-5)
            assert out["total_loss"] == pytest.approx(o_loss + o_reg, rel=1e-5)
            for n, og in o_g.items():
                err = np.linalg.norm(g[n].astype(np.float64) - og)
                assert err <= GTOL * np.linalg.norm(og) + 1e-7, "step %d, %s: rel err %.3g" % (k, n, rel[n])
            lr = exponential_decay(k, 0.01, 2, 0.5, staircase=True)
            rates.append(lr)
            assert out["learning_rate"] == pytest.approx(lr, rel=1e-12) and out["step"] == k + 1
            adam_step(ref, {n: g[n].astype(np.float64) for n in ref}, rm, rv, k, *_abi_f32(lr, 0.9, 0.999, 1e-7))
            got, gm, gv = tr.params(), _named(eng, tr.m.cpu().numpy()), _named(eng, tr.v.cpu().numpy())
            for n in ref:
                assert not np.array_equal(got[n], p_k[n]), n
                np.testing.assert_allclose(got[n], ref[n], rtol=1e-5, atol=1e-6, err_msg="step %d, %s" % (k, n))
                np.testing.assert_allclose(gm[n], rm[n], rtol=1e-5, atol=1e-6, err_msg="step %d, m of %s" % (k, n))
                np.testing.assert_allclose(gv[n], rv[n], rtol=1e-5, atol=1e-6, err_msg="step %d, v of %s" % (k, n))
        assert rates == [0.01, 0.01, 0.005, 0.005][:steps]
    finally:   # train_prepared closes the batch it ran; a failed step leaves the later ones open
        for b, _ in prepared:
            b.close()
        eng.close()
