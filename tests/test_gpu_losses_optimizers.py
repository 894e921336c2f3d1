"""The Keras losses and optimizers beside MeanSquaredError / Adam on the GPU (ign_loss,
ign_optimizer_step; Engine.loss, Engine.optimizer_step, Trainer, EdgeCutTraining) against the float64
restatement in tests/keras_restated.py.

Bounds: a loss value within 1e-5 relative and the parameters / slots after an update within rtol 1e-5,
atol 1e-6 (test_gpu_training.py's bounds for the MSE loss and the Adam update); dpred element-wise within
rtol 1e-5 and exactly 0 where the loss's derivative is defined as 0; gradients per tensor within GTOL."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from ignnition_amd import _lib, model_examples, partition, synthetic, workloads
from ignnition_amd.engine import Batch, Engine, MPPlan, device_count
from ignnition_amd.json_operations import Model_information
from ignnition_amd.training import Trainer
from oracle.train_oracle import TorchOracle, exponential_decay
from tests import keras_restated as kr
from tests.test_gpu_training import GTOL, _engine_grads

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _model(kind, hidden, iterations):
    desc = (model_examples.qsize(hidden=hidden, iterations=iterations) if kind == "qsize"
            else model_examples.routenet(hidden=hidden, iterations=iterations))
    _, dims, _ = workloads.model(kind)
    return desc, dims, Model_information(copy.deepcopy(desc), dims)


def _flat(eng):
    """The flat parameter buffer, alignment gaps included."""
    out = np.empty(eng.n_params, np.float32)
    _lib.check(_lib.lib.ign_plan_get_params(eng.handle, out.ctypes.data_as(C.c_void_p)))
    return out


# ---------------------------------------------------------------------------------------------
# the loss kernel
SIZES = [1, 255, 257, 65539]   # 65539: one full pass of the 256 x 256 grid and a tail (the loop's second trip)
ONE_UP, ONE_DOWN = F32(1.0000001), F32(0.99999994)   # the float32 neighbours of 1
EPS32_HALF = F32(5e-8)


@pytest.fixture(scope="module")
def loss_engine():
    _, _, mi = _model("routenet", 16, 2)
    eng = Engine(MPPlan.from_model_info(mi), 0)
    yield eng
    eng.close()


def _plant(p, y, pairs, at=5):
    for k, (a, b) in enumerate(pairs):
        if at + k < p.size:
            p[at + k], y[at + k] = a, b


def _loss_inputs(name, n):
    """Seeded O(1) float32 p, y in the loss's domain with its kink values at fixed indices."""
    rng = np.random.default_rng(1000 * kr.LOSSES.index(name) + n % 1000)
    if name == "BinaryCrossentropy":
        p, y = rng.uniform(0.01, 0.99, n).astype(F32), rng.uniform(0.0, 1.0, n).astype(F32)
        _plant(p, y, [(a, b) for a in (-0.5, 0.0, 1.0, 1.5) for b in (0.0, 1.0, 0.3)])
    elif name in ("Poisson", "MeanSquaredLogarithmicError", "MeanAbsolutePercentageError"):
        p, y = rng.uniform(0.05, 3.0, n).astype(F32), rng.uniform(0.05, 3.0, n).astype(F32)
        _plant(p, y, [(0.0, 1.5), (EPS32_HALF, 0.7), (1.25, 0.0), (0.0, 0.0), (0.6, 0.6)])
    else:
        p, y = rng.normal(0, 1.5, n).astype(F32), rng.normal(0, 1.5, n).astype(F32)
        _plant(p, y, [(0.75, 0.75), (1.0, 0.0), (-1.0, 0.0), (ONE_UP, 0.0), (ONE_DOWN, 0.0), (0.0, ONE_UP),
                      (0.0, ONE_DOWN), (2.5, 1.5), (0.0, 0.0)])
    return p, y


def _run_loss(eng, kind, p, y, want_loss=True):
    pd, yd = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
    d = torch.full_like(pd, float("nan"))
    torch.cuda.synchronize()   # the fill runs on torch's stream, the loss on the plan's: nothing else orders them
    loss = eng.loss(kind, pd, yd, d, want_loss=want_loss)
    torch.cuda.synchronize()
    return loss, d.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", kr.LOSSES)
def test_loss_kernel(loss_engine, name, n):
    kind = kr.LOSSES.index(name)
    p, y = _loss_inputs(name, n)
    loss, d = _run_loss(loss_engine, kind, p, y)
    ref, dref = kr.loss(name, p, y), kr.dpred(name, p, y)
    zero = kr.dpred_is_zero(name, p, y)
    rel = np.abs(d - dref) / np.maximum(np.abs(dref), 1e-300)
    rel[zero] = 0
    worst = int(np.argmax(rel))
    print("%s n=%d: loss %.12g (float64 %.12g, rel %.3g); dpred worst rel %.3g at %d (p %.9g, y %.9g); %d exact zeros"
          % (name, n, loss, ref, abs(loss - ref) / abs(ref), rel[worst], worst, p[worst], y[worst], int(zero.sum())))
    assert loss == pytest.approx(ref, rel=1e-5)
    assert np.all(d[zero] == 0.0)
    np.testing.assert_allclose(d, dref, rtol=1e-5, atol=0)
    _, d2 = _run_loss(loss_engine, kind, p, y, want_loss=False)
    np.testing.assert_array_equal(d2, d)


@pytest.mark.parametrize("n", SIZES)
def test_loss_kind_0_is_mse_loss(loss_engine, n):
    """ign_mse_loss forwards to ign_loss with kind 0, and Engine.mse_loss is Engine.loss(0): both give
    the loss and dpred of kind 0 bit for bit."""
    p, y = _loss_inputs("MeanSquaredError", n)
    pd, yd = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
    l1, d1 = _run_loss(loss_engine, 0, p, y)
    d0 = torch.empty_like(pd)
    l0 = loss_engine.mse_loss(pd, yd, d0)
    assert l0 == l1
    np.testing.assert_array_equal(d0.cpu().numpy(), d1)
    d0 = torch.empty_like(pd)
    out = C.c_double()
    _lib.check(_lib.lib.ign_mse_loss(loss_engine.handle, C.c_void_p(pd.data_ptr()), C.c_void_p(yd.data_ptr()), n,
                                     C.c_void_p(d0.data_ptr()), C.byref(out)))
    assert out.value == l1
    np.testing.assert_array_equal(d0.cpu().numpy(), d1)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])   # the block edge; 65537: one thread's second trip
def test_mse_dpred_is_the_float32_expression(loss_engine, n):
    """MeanSquaredError's dpred against numpy, independent of the engine: one correctly rounded float32
    division, subtraction and multiplication on both sides (nothing to contract), so bit for bit."""
    p, y = _loss_inputs("MeanSquaredError", n)
    loss, d = _run_loss(loss_engine, 0, p, y)
    ref = (F32(2) / F32(n)) * (p - y)
    assert ref.dtype == np.float32
    np.testing.assert_array_equal(d.view(np.uint32), ref.view(np.uint32))
    assert loss == pytest.approx(kr.loss("MeanSquaredError", p, y), rel=1e-5)


def test_loss_kind_out_of_range(loss_engine):
    x = torch.zeros(4, device="cuda")
    with pytest.raises(_lib.EngineError) as ei:
        loss_engine.loss(8, x, x, torch.empty_like(x))
    assert ei.value.code == -1


# ---------------------------------------------------------------------------------------------
# the optimizer kernel
OPT_CASES = [("SGD", {}, 0.01), ("SGD", {"momentum": 0.9}, 0.01), ("SGD", {"momentum": 0.9, "nesterov": True}, 0.01),
             ("RMSprop", {}, 0.01), ("RMSprop", {"centered": True}, 0.01), ("RMSprop", {"momentum": 0.9}, 0.01),
             ("RMSprop", {"centered": True, "momentum": 0.9}, 0.01), ("Adagrad", {}, 0.01), ("Adadelta", {}, 1.0),
             ("Adamax", {}, 0.01)]
_IDS = ["%s%s" % (n, "".join("-" + k for k in g)) for n, g, _ in OPT_CASES]
_GRADS = {}


def _abi_hyper(name, given):
    """The hyper-parameters as the C ABI carries them (float): the restatement is fed the same values."""
    return {k: (float(F32(v)) if isinstance(v, float) else v) for k, v in kr.hyper(name, **given).items()}


def _desc(name, h):
    return _lib.OptimizerDesc(kind=kr.OPTIMIZERS.index(name), nesterov=int(h.get("nesterov", False)),
                              centered=int(h.get("centered", False)), reserved=0, momentum=h.get("momentum", 0.0),
                              rho=h.get("rho", 0.0), beta_1=h.get("beta_1", 0.0), beta_2=h.get("beta_2", 0.0),
                              epsilon=h.get("epsilon", 0.0),
                              initial_accumulator_value=h.get("initial_accumulator_value", 0.0))


def _slots(name, h, n_params):
    desc = _desc(name, h)
    n, init = C.c_int32(), C.c_float()
    _lib.check(_lib.lib.ign_optimizer_num_slots(C.byref(desc), C.byref(n), C.byref(init)))
    assert n.value == kr.num_slots(name, h)
    return desc, [torch.full((n_params,), init.value, dtype=torch.float32, device="cuda") for _ in range(n.value)]


def _real_grads(kind):
    """Once per model: RouteNet H = 16 / Q-size H = 32 on two NSFNET graphs, _engine_grads' recipe."""
    if kind not in _GRADS:
        desc, dims, mi = _model(kind, 32 if kind == "qsize" else 16, 2 if kind == "qsize" else 3)
        graphs, labels = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", g, qsize=kind == "qsize")
                                                     for g in range(2)])
        prm = MPPlan.from_model_info(mi).init_params(1, bias_scale=0.1)
        eng, b, _, _, _, grads = _engine_grads(desc, dims, graphs, labels, prm)
        _GRADS[kind] = (mi, prm, graphs, grads.cpu().numpy())
        b.close()
        eng.close()
    return _GRADS[kind]


def _three_steps(kind, name, given, lr):
    mi, prm, _, g = _real_grads(kind)
    eng = Engine(MPPlan.from_model_info(mi), 0)
    try:
        eng.set_params(prm)
        h = _abi_hyper(name, given)
        desc, slots = _slots(name, h, eng.n_params)
        gd = torch.from_numpy(g).cuda()
        w = _flat(eng).astype(np.float64)
        w0 = w.copy()
        ref_slots = kr.init_slots(name, h, w.size)
        for it in range(3):
            eng.optimizer_step(desc, gd, slots, it, lr)
            kr.optimizer_step(name, h, w, g.astype(np.float64), ref_slots, it, float(F32(lr)))
        torch.cuda.synchronize()
        got = _flat(eng)
        assert np.abs(w - w0).max() > 1e-4   # the update is far above the absolute bound it is held to
        np.testing.assert_allclose(got, w, rtol=1e-5, atol=1e-6)
        for k, (s, r) in enumerate(zip(slots, ref_slots)):
            np.testing.assert_allclose(s.cpu().numpy(), r, rtol=1e-5, atol=1e-6, err_msg="slot %d" % k)
    finally:
        eng.close()


@pytest.mark.parametrize("name,given,lr", OPT_CASES, ids=_IDS)
def test_optimizer_kernel(name, given, lr):
    _three_steps("routenet", name, given, lr)


def test_optimizer_kernel_other_tail():
    _three_steps("qsize", "RMSprop", {"centered": True, "momentum": 0.9}, 0.01)


@pytest.mark.parametrize("name,given,lr", OPT_CASES, ids=_IDS)
def test_zero_gradient_leaves_the_buffer_unchanged(name, given, lr):
    mi, prm, _, _ = _real_grads("routenet")
    eng = Engine(MPPlan.from_model_info(mi), 0)
    try:
        eng.set_params(prm)
        h = _abi_hyper(name, given)
        desc, slots = _slots(name, h, eng.n_params)
        before = _flat(eng)
        used = np.zeros(eng.n_params, bool)
        for _, shape, off in eng.layout:
            used[off:off + int(np.prod(shape))] = True
        assert not used.all() and not before[~used].any()   # the alignment gaps exist and hold zeros
        eng.optimizer_step(desc, torch.zeros(eng.n_params, device="cuda"), slots, 0, lr)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_flat(eng).view(np.uint32), before.view(np.uint32))
        init = h["initial_accumulator_value"] if name == "Adagrad" else 0.0
        for s in slots:
            assert bool((s == float(F32(init))).all())
    finally:
        eng.close()


def test_forward_follows_the_update():
    """The repack follows ign_optimizer_step: a forward after an SGD step is a fresh engine's."""
    mi, prm, graphs, g = _real_grads("routenet")
    eng, fresh = Engine(MPPlan.from_model_info(mi), 0), Engine(MPPlan.from_model_info(mi), 0)
    try:
        eng.set_params(prm)
        before = Batch(eng, graphs).forward()
        h = _abi_hyper("SGD", {})
        desc, slots = _slots("SGD", h, eng.n_params)
        eng.optimizer_step(desc, torch.from_numpy(g).cuda(), slots, 0, 0.01)
        fresh.set_params(eng.get_params())
        after = Batch(eng, graphs).forward()
        assert not np.array_equal(after, before)
        np.testing.assert_array_equal(after, Batch(fresh, graphs).forward())
    finally:
        eng.close()
        fresh.close()


def test_optimizer_kind_0_is_adam_step():
    """ign_adam_step fills a desc of kind 0 from its loose hyper-parameters and forwards to
    ign_optimizer_step: two steps through either give the same parameters, m and v bit for bit."""
    mi, prm, _, g = _real_grads("routenet")
    a, b = Engine(MPPlan.from_model_info(mi), 0), Engine(MPPlan.from_model_info(mi), 0)
    try:
        gd = torch.from_numpy(g).cuda()
        h = {"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7}
        desc, slots = _slots("Adam", h, a.n_params)
        m, v = torch.zeros_like(gd), torch.zeros_like(gd)
        for e in (a, b):
            e.set_params(prm)
        for it in range(2):
            a.optimizer_step(desc, gd, slots, it, 0.01)
            b.adam_step(gd, m, v, it, 0.01)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_flat(a).view(np.uint32), _flat(b).view(np.uint32))
        assert torch.equal(slots[0], m) and torch.equal(slots[1], v)
    finally:
        a.close()
        b.close()


def test_optimizer_step_argument_checks():
    mi, prm, _, g = _real_grads("routenet")
    eng = Engine(MPPlan.from_model_info(mi), 0)
    try:
        eng.set_params(prm)
        h = _abi_hyper("RMSprop", {"centered": True})
        desc, slots = _slots("RMSprop", h, eng.n_params)
        with pytest.raises(_lib.EngineError) as ei:
            eng.optimizer_step(desc, torch.from_numpy(g).cuda(), slots[:1], 0, 0.01)
        assert ei.value.code == -1 and "slot" in str(ei.value)
        # Adam takes the same checks (and leaves the parameters alone when one fails)
        before = _flat(eng)
        gd = torch.from_numpy(g).cuda()
        h = {"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7}
        desc, slots = _slots("Adam", h, eng.n_params)
        assert desc.kind == 0
        bad = _desc("Adam", h)
        bad.reserved = 1
        for d, s, it, word in ((desc, slots[:1], 0, "slot"), (desc, slots + slots[:1], 0, "slot"),
                               (desc, [slots[0], 0], 0, "slot buffer 1 is null"), (bad, slots, 0, "reserved"),
                               (desc, slots, -1, "negative iteration")):
            with pytest.raises(_lib.EngineError) as ei:
                eng.optimizer_step(d, gd, s, it, 0.01)
            assert ei.value.code == -1 and word in str(ei.value), word
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_flat(eng).view(np.uint32), before.view(np.uint32))
        assert not any(bool(s.any()) for s in slots)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------
# end to end
def _torch_loss(name, pred, y):
    d = pred - y
    if name == "Huber":
        return torch.where(d.abs() <= 1.0, d * d / 2.0, d.abs() - 0.5).mean()
    assert name == "MeanAbsoluteError"
    return d.abs().mean()


def _named(eng, flat):
    return {n: flat[off:off + int(np.prod(shape))].reshape(shape) for n, shape, off in eng.layout}


@pytest.mark.parametrize("loss,opt", [("Huber", {"type": "SGD", "momentum": 0.9}),
                                      ("MeanAbsoluteError", {"type": "RMSprop"})])
def test_trainer_end_to_end(loss, opt):
    """Two Trainer steps on RouteNet H = 16, two NSFNET graphs each.  Step k, from P_k and the slots as they
    are: the loss within 1e-5 relative and every gradient tensor within GTOL of float64 autograd of the restated
    loss + regularization at P_k; P_k+1 and the slots within rtol 1e-5 / atol 1e-6 of the restated optimizer
    fed the engine's own gradient (so gradient error does not compound into the optimizer check)."""
    desc, dims, _ = _model("routenet", 16, 3)
    desc["learning_options"] = {"loss": loss, "optimizer": dict(opt)}
    mi = Model_information(copy.deepcopy(desc), dims)
    data = [workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", 2 * k + g) for g in range(2)])
            for k in range(2)]
    name = opt["type"]
    h = _abi_hyper(name, {k: v for k, v in opt.items() if k != "type"})
    rate = kr.DEFAULTS[name]["learning_rate"]
    tr = Trainer(mi, params=MPPlan.from_model_info(mi).init_params(7, bias_scale=0.1))
    eng = tr.engine
    try:
        assert tr.m is None and tr.v is None and len(tr.slots) == kr.num_slots(name, h)
        for k, (graphs, labels) in enumerate(data):
            p_k = tr.params()
            w = _flat(eng).astype(np.float64)
            ref_slots = [s.cpu().numpy().astype(np.float64) for s in tr.slots]
            out = tr.train_step(graphs, labels)
            o = TorchOracle(desc, dims, p_k)
            y = torch.tensor(np.concatenate([np.asarray(l, np.float64).reshape(-1) for l in labels]))
            o_loss, o_reg = _torch_loss(loss, o.forward(graphs), y), o.regularization()
            (o_loss + o_reg).backward()
            o_loss, o_reg = float(o_loss.detach()), float(o_reg.detach())
            gflat = tr.grads.cpu().numpy()
            g = _named(eng, gflat)
            rel = {}
            for n, v in o.p.items():
                og = v.grad.numpy() if v.grad is not None else np.zeros(v.shape)
                err = np.linalg.norm(g[n].astype(np.float64) - og)
                rel[n] = err / max(np.linalg.norm(og), 1e-30)
                assert err <= GTOL * np.linalg.norm(og) + 1e-7, "step %d, %s: rel err %.3g" % (k, n, rel[n])
            worst = max(rel, key=rel.get)
            print("step %d: loss %.9g (oracle %.9g), worst gradient tensor %s %.3g" % (k, out["loss"], float(o_loss), worst, rel[worst]))
            assert out["loss"] == pytest.approx(float(o_loss), rel=1e-5)
            assert out["regularization_loss"] == pytest.approx(float(o_reg), rel=1e-5)
            assert out["learning_rate"] == rate and out["step"] == k + 1
            kr.optimizer_step(name, h, w, gflat.astype(np.float64), ref_slots, k, float(F32(rate)))
            got = _flat(eng)
            assert not np.array_equal(got, w.astype(np.float32))
            np.testing.assert_allclose(got, w, rtol=1e-5, atol=1e-6, err_msg="step %d" % k)
            for i, (s, r) in enumerate(zip(tr.slots, ref_slots)):
                np.testing.assert_allclose(s.cpu().numpy(), r, rtol=1e-5, atol=1e-6, err_msg="step %d, slot %d" % (k, i))
        # evaluate reports the configured loss, in float64 on the engine's predictions
        graphs, labels = data[0]
        ev = tr.evaluate([data[0]])
        b = Batch(eng, graphs)
        pred = b.forward().reshape(-1)
        b.close()
        yv = np.concatenate([np.asarray(l, np.float64).reshape(-1) for l in labels])
        assert ev["loss"] == pytest.approx(kr.loss(loss, pred, yv), rel=1e-12)
        assert ev["loss"] != pytest.approx(kr.loss("MeanSquaredError", pred, yv), rel=1e-3)
        # both losses are 1-Lipschitz means, the predictions hold _check_grads' 1e-4 bound against the oracle
        o_pred = TorchOracle(desc, dims, tr.params()).forward(graphs).detach().numpy()
        assert abs(ev["loss"] - kr.loss(loss, o_pred, yv)) <= 1e-4 * (1 + np.abs(o_pred).max())
    finally:
        eng.close()


def test_default_configuration_is_untouched():
    """MeanSquaredError + Adam + ExponentialDecay (the stock RouteNet description): two Trainer steps give
    parameters, m and v bitwise equal to the mse_loss / backward / adam_step calls made by hand."""
    desc, dims, mi = _model("routenet", 32, 8)
    sched = desc["learning_options"]["optimizer"]["schedule"]
    data = [workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", 2 * k + g) for g in range(2)])
            for k in range(2)]
    prm = MPPlan.from_model_info(mi).init_params(7, bias_scale=0.1)
    tr = Trainer(mi, params=prm)
    eng = Engine(MPPlan.from_model_info(mi), 0)
    try:
        eng.set_params(prm)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
        m, v = torch.zeros_like(grads), torch.zeros_like(grads)
        assert tr.slots[0] is tr.m and tr.slots[1] is tr.v
        for k, (graphs, labels) in enumerate(data):
            out = tr.train_step(graphs, labels)
            b = Batch(eng, graphs)
            b.enable_training()
            b.forward_train(to_host=False)
            y = torch.from_numpy(np.concatenate([np.asarray(l, np.float32).reshape(-1) for l in labels])).cuda()
            dpred = torch.empty_like(y)
            loss = eng.mse_loss(b.predictions_ptr(), y, dpred)
            b.backward(dpred, grads)
            lr = exponential_decay(k, float(sched["initial_learning_rate"]), float(sched["decay_steps"]),
                                   float(sched["decay_rate"]), staircase=sched.get("staircase", False))
            eng.adam_step(grads, m, v, k, lr, 0.9, 0.999, 1e-7)
            b.close()
            torch.cuda.synchronize()
            assert out["loss"] == loss and out["learning_rate"] == lr
            np.testing.assert_array_equal(_flat(tr.engine).view(np.uint32), _flat(eng).view(np.uint32))
            assert torch.equal(tr.m, m) and torch.equal(tr.v, v) and bool(m.any())
    finally:
        eng.close()
        tr.engine.close()


# ---------------------------------------------------------------------------------------------
# edge cut
def test_partitioned_training_step_with_mean_absolute_error():
    """test_gpu_edge_cut.py's two-partition loopback training step (sum MPs) with MeanAbsoluteError: the
    predictions bit for bit, the loss and the summed gradient at that test's tolerances against the whole-graph
    engine run with the same loss."""
    kind = kr.LOSSES.index("MeanAbsoluteError")
    world = 2
    desc, dims, _, graphs, labels = workloads.make_synthetic_inputs(n_nodes=2500, hidden=32, iterations=2, window=96)
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(12, bias_scale=0.1))
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    b = Batch(eng, graphs)
    b.enable_training()
    pred = b.forward_train().reshape(-1)
    lab = np.asarray(labels[0], np.float32).reshape(-1)
    y = torch.from_numpy(lab).cuda()
    dpred = torch.empty_like(y)
    loss = eng.loss(kind, b.predictions_ptr(), y, dpred)
    assert loss == pytest.approx(kr.loss("MeanAbsoluteError", pred, lab), rel=1e-5)
    g_whole = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    b.backward(dpred, g_whole)
    torch.cuda.synchronize()
    b.close()
    parts = [partition.local_part(graphs[0], plan, r, world) for r in range(world)]
    comm = partition.LoopbackComm(world)
    partition.exchange_requests(parts, comm)
    ranges = parts[0].ranges["node"]
    tr = partition.EdgeCutTraining(eng, parts, comm)
    try:
        loss_p, g_p, preds = tr.step([lab[ranges[r]:ranges[r + 1]] for r in range(world)], loss_kind=kind)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(np.concatenate([p.reshape(-1) for p in preds]), pred)
        assert loss_p == pytest.approx(loss, rel=1e-6)
        gw, gp = g_whole.double(), g_p.double()
        assert float(torch.linalg.norm(gp - gw)) <= 1e-5 * float(torch.linalg.norm(gw))
        # and not the MSE step's
        loss_mse, g_mse, _ = tr.step([lab[ranges[r]:ranges[r + 1]] for r in range(world)])
        assert loss_mse != pytest.approx(loss, rel=1e-3)
        assert float(torch.linalg.norm(g_mse.double() - gw)) > 1e-3 * float(torch.linalg.norm(gw))
    finally:
        tr.close()
        torch.cuda.synchronize()
