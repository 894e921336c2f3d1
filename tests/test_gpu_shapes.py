"""The table of tests/shape_cases.py on the GPU: graphs whose path, link, node and message counts sit on the
kernels' row-tile, block, group and chunk edges and on the lane-walk / segmented-sum switch, H = 32 (a few
at 16 and 64), T = 2.

Every check is an existing helper with its own bound: test_gpu_parity's _resident_vs_batched and _close
(TOL), test_gpu_training's _check_grads (GTOL per tensor, loss and l2 at 1e-5), test_gpu_predict_nets'
_forward_twice, test_gpu_dropout's _train / _assert_grads and its mask assertion, and the loss bound of
test_gpu_losses_optimizers (1e-5 relative against tests/keras_restated.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from ignnition_amd import model_examples
from ignnition_amd.engine import Batch, Engine, device_count, dropout_keep
from tests import dropout_cases as dc
from tests import keras_restated as kr
from tests import shape_cases as sc
from tests.predict_cases import FUSED, PREDICT_CASES, predict_model
from tests.test_gpu_dropout import GRAD_CASES, SEED as DSEED, STEP, _assert_grads, _forward_train, _mask_model, _train
from tests.test_gpu_losses_optimizers import _run_loss
from tests.test_gpu_parity import _close, _resident_vs_batched, _scaled_err
from tests.test_gpu_predict_nets import _forward_twice
from tests.test_gpu_training import _check_grads, _engine_grads

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(sc.SHAPES)
TS_CASES = ["p33", "p129", "p257"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _set_env(monkeypatch, name):
    for k, v in sc.SHAPES[name].env:
        monkeypatch.setenv(k, v)


def _predictions(plan, prm, batches):
    """The flat predictions of each batch (a list of graphs) on one fresh engine under the current environment."""
    eng = Engine(plan, 0)
    eng.set_params(prm)
    outs = []
    for graphs in batches:
        b = Batch(eng, graphs)
        outs.append(b.forward().reshape(-1).copy())
        b.close()
    eng.close()
    return outs


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_forward_resident_and_batched(monkeypatch, name):
    """_resident_vs_batched on every entry: IGN_RESIDENT=1 and =0 bitwise equal in predictions and final
    states, within TOL of the float64 oracle, replayed bitwise from the captured hipGraph.  Which way the
    IGN_RESIDENT=1 run went is read from ign_batch_resident_info first: the resident launch is there for
    H = 32 without the windowed sum and nowhere else (engine.cpp's resident_plan_shape), and its
    segmented rows are the union rows of >= 64 messages."""
    _set_env(monkeypatch, name)
    s = sc.SHAPES[name]
    desc, dims, mi, plan, graphs, _, prm = sc.case_inputs(name)
    monkeypatch.setenv("IGN_RESIDENT", "1")
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    probe = b.resident_info()
    b.close()
    eng.close()
    print("%s: resident %s" % (name, {k: probe.get(k) for k in ("active", "form", "union_tiles", "seg_rows")}))
    assert probe["active"] == int(s.hidden == 32 and ("IGN_SUM_WINDOW", "1") not in s.env), probe
    info = _resident_vs_batched(monkeypatch, desc, dims, mi, graphs, seed=sc.SEED, bias=sc.BIAS,
                                resident=bool(probe["active"]))
    if info["active"]:
        rows = [("link", "dst_adj_paths_links")] + ([("node", "dst_adj_paths_nodes")] if s.kind == "qsize" else [])
        seg = sum(int((np.bincount(g[a], minlength=g["num_" + e]) >= 64).sum()) for g in graphs for e, a in rows)
        assert info["seg_rows"] == seg, info


@pytest.mark.parametrize("name", ALL)
def test_placement_and_poisoned_scratch(monkeypatch, name):
    """Each graph's predictions are the same bits alone and at every position of its batch entry (the
    entry's rotations), and the entry's are the same bits on NaN-poisoned scratch (IGN_POOL_POISON=1);
    the default run is within TOL of the cached float64 oracle."""
    _set_env(monkeypatch, name)
    _, _, _, plan, graphs, _, prm = sc.case_inputs(name)
    n = len(graphs)
    rotations = [graphs[r:] + graphs[:r] for r in range(n)]
    outs = _predictions(plan, prm, rotations + [[g] for g in graphs])
    whole, alone = outs[0], outs[n:]
    print("%s: max scaled error vs float64 oracle %.3g" % (name, _scaled_err(whole, sc.reference(name))))
    _close(whole, sc.reference(name))
    np.testing.assert_array_equal(whole, np.concatenate(alone))
    for r in range(1, n):
        np.testing.assert_array_equal(outs[r], np.concatenate(alone[r:] + alone[:r]), err_msg="rotation %d" % r)
    monkeypatch.setenv("IGN_POOL_POISON", "1")
    np.testing.assert_array_equal(_predictions(plan, prm, [graphs])[0], whole)


@pytest.mark.parametrize("name", ALL)
def test_gradients(monkeypatch, name):
    """_check_grads against float64 autograd, then the same bits with host-built transposed CSRs
    (IGN_TRAIN_CSR_GPU=0) and with the per-MP training forward (IGN_RESIDENT_TRAIN=0)."""
    _set_env(monkeypatch, name)
    desc, dims, _, _, graphs, labels, prm = sc.case_inputs(name)
    print(name)
    eng, b, grads = _check_grads(desc, dims, graphs, labels, prm, oracle=sc.grad_reference(name))
    base = grads.cpu().numpy()
    b.close()
    eng.close()
    assert np.abs(base).sum() > 0
    for switch in ("IGN_TRAIN_CSR_GPU", "IGN_RESIDENT_TRAIN"):
        with monkeypatch.context() as m:
            m.setenv(switch, "0")
            eng, b, _, _, _, g = _engine_grads(desc, dims, graphs, labels, prm)
            got = g.cpu().numpy()
            b.close()
            eng.close()
        np.testing.assert_array_equal(got, base, err_msg=switch + "=0")


# ---------------------------------------------------------------------------------------------
# ts_plan's chunks: IGN_TS_MIN_ROWS is read once per process, so one child process runs the three entries
def _ts_child(out_path):
    res = {}
    for name in TS_CASES:
        desc, dims, _, _, graphs, labels, prm = sc.case_inputs(name)
        eng, b, pred, loss, _, grads = _engine_grads(desc, dims, graphs, labels, prm)
        res[name + "/grads"], res[name + "/pred"], res[name + "/loss"] = grads.cpu().numpy(), pred.reshape(-1), np.float64(loss)
        b.close()
        eng.close()
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def ts32(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ts32") / "grads.npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.test_gpu_shapes", out]
    run = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, IGN_TS_MIN_ROWS="32"), capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    return dict(np.load(out))


@pytest.mark.parametrize("name", TS_CASES)
def test_gradients_with_32_row_chunks(ts32, name):
    """IGN_TS_MIN_ROWS=32: the weight-gradient row contractions split their partials into chunks of 32
    rows with a short last one (where the rows are the paths, P = 33: 32 + 1; 129: 4 x 32 + 1; 257:
    8 x 32 + 1).  Every tensor within GTOL of float64 autograd, the loss at 1e-5; over the three entries the
    chunking changes at least one gradient bit (the knob reached the child process)."""
    desc, dims, _, plan, graphs, labels, prm = sc.case_inputs(name)
    o_loss, _, o_g, o_pred = sc.grad_reference(name)
    eng = Engine(plan, 0)
    layout = eng.layout
    eng.close()
    g = ts32[name + "/grads"]
    named = {n: g[off:off + int(np.prod(shape))].reshape(shape) for n, shape, off in layout}
    np.testing.assert_allclose(ts32[name + "/pred"], o_pred, rtol=1e-4, atol=1e-4)
    assert float(ts32[name + "/loss"]) == pytest.approx(o_loss, rel=1e-5)
    _assert_grads(named, o_g, name + " IGN_TS_MIN_ROWS=32: ")
    if name == TS_CASES[-1]:
        differs = []
        for c in TS_CASES:
            d, dm, _, _, gr, lb, pr = sc.case_inputs(c)
            eng, b, _, _, _, base = _engine_grads(d, dm, gr, lb, pr)
            differs.append(not np.array_equal(base.cpu().numpy(), ts32[c + "/grads"]))
            b.close()
            eng.close()
        print("gradient bits differ from the 128-row chunks:", dict(zip(TS_CASES, differs)))
        assert any(differs)


# ---------------------------------------------------------------------------------------------
# Dense stacks at the row edges
DENSE = ["selu", "four_layer", "odd_widths", "out3", "one_layer", "nobias_hidden"]
DENSE_P = [1, 16, 17, 33, 128, 129]


def _t2(desc):
    desc["message_passing"]["num_iterations"] = sc.ITERATIONS
    return desc


@functools.lru_cache(maxsize=None)
def _dense_case(case, P):
    """A predict-network case on the P sweep's graph: its inputs and both float64 references, once."""
    from oracle.dense_forward import DenseOracle
    from oracle.train_oracle import TorchOracle
    desc, dims = _t2(predict_model(case, hidden=32)), sc.dims("routenet")
    graphs = [sc.graph(sc.P_GRAPH[P])]
    _, plan, labels, prm = sc.inputs_for(desc, dims, graphs, units=PREDICT_CASES[case][-1][0])
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    ref.setflags(write=False)
    o = TorchOracle(desc, dims, prm).loss_and_grads(graphs, labels)
    sc.well_conditioned(labels, o[3])
    return desc, dims, plan, graphs, labels, prm, ref, o


@pytest.mark.parametrize("P", DENSE_P)
@pytest.mark.parametrize("case", DENSE)
def test_dense_stack_forward(case, P):
    """One fused launch (selu) or one launch per layer, bitwise repeatable, within TOL of DenseOracle."""
    desc, dims, plan, graphs, _, prm, ref, _ = _dense_case(case, P)
    layers = PREDICT_CASES[case]
    assert P == 1 or np.ptp(ref) > 1e-3, "%s: the oracle's predictions are constant" % case
    out = _forward_twice(plan, prm, graphs, 1 if case in FUSED else len(layers))
    assert out.shape == (P, layers[-1][0])
    print("%s P %d: max scaled error vs float64 oracle %.3g" % (case, P, _scaled_err(out, ref)))
    _close(out, ref)


@pytest.mark.parametrize("P", DENSE_P)
@pytest.mark.parametrize("case", DENSE)
def test_dense_stack_gradients(case, P):
    desc, dims, _, graphs, labels, prm, _, o = _dense_case(case, P)
    print(case, P)
    eng, b, _ = _check_grads(desc, dims, graphs, labels, prm, oracle=o)
    b.close()
    eng.close()


MESSAGES = {1: sc.G(1, 1, 1), 16: sc.G(16, 2, 1), 17: sc.G(17, 5, 1), 65: sc.G(65, 3, 1)}   # length-1 paths: P messages


@pytest.mark.parametrize("count", sorted(MESSAGES))
def test_message_network_rows(count):
    """test_gradients_message_networks' first parameter set (hs_source | hs_dest -> 24 selu -> 32 selu on
    the path -> link sum MP, l2 0.01 on its first kernel) with 1, 16, 17 and 65 message rows in all."""
    from oracle.dense_forward import DenseOracle
    from oracle.train_oracle import TorchOracle
    desc = model_examples.routenet_message_net(inputs=("hs_source", "hs_dest"), units=(24, 32), activation="selu",
                                               iterations=sc.ITERATIONS)
    [n for n in desc["neural_networks"] if n["nn_name"] == "message_nn"][0]["nn_architecture"][0]["kernel_regularizer"] = 0.01
    dims, graphs = sc.dims("routenet"), [sc.graph(MESSAGES[count])]
    assert len(graphs[0]["src_adj_paths_links"]) == count
    _, plan, labels, prm = sc.inputs_for(desc, dims, graphs)
    (out,) = _predictions(plan, prm, [graphs])
    _close(out, DenseOracle(desc, dims, prm).forward(graphs))
    o = TorchOracle(desc, dims, prm).loss_and_grads(graphs, labels)
    sc.well_conditioned(labels, o[3])
    eng, b, _ = _check_grads(desc, dims, graphs, labels, prm, oracle=o)
    b.close()
    eng.close()


# ---------------------------------------------------------------------------------------------
# Dropout
@pytest.mark.parametrize("P", [1, 17, 129])
def test_dropout_mask_rows(P):
    """test_device_mask_is_the_host_function's assertion on P x 7 outputs: zero exactly where
    ign_dropout_keep drops, elsewhere bitwise float32(y) * float32(1 / (1 - rate))."""
    rate = 0.25
    dims, graphs = sc.dims("routenet"), [sc.graph(sc.P_GRAPH[P])]
    _, plan, _, prm = sc.inputs_for(_t2(_mask_model(rate)), dims, graphs, units=7)
    (y,) = _forward_train(_t2(_mask_model(0.0)), dims, graphs, prm, [None])
    (z,) = _forward_train(_t2(_mask_model(rate)), dims, graphs, prm, [(DSEED, STEP)])
    assert y.shape == (P, 7) and np.isfinite(y).all()
    keep = dropout_keep(DSEED, 0, STEP, P, 7, rate).astype(bool)
    assert (z[~keep] == 0.0).all()
    np.testing.assert_array_equal(z[keep], (y * np.float32(1.0 / (1.0 - rate)))[keep])


@pytest.mark.parametrize("P", [1, 17, 129])
def test_dropout_gradient_rows(P):
    """dropout_cases' four_layer (Dropout 0.5 before Dense 1 and Dense 3) against float64 autograd with the
    ign_dropout_keep masks of P rows."""
    desc = _t2(GRAD_CASES["four_layer"]())
    dims, graphs = sc.dims("routenet"), [sc.graph(sc.P_GRAPH[P])]
    _, plan, labels, prm = sc.inputs_for(desc, dims, graphs)
    pred, _, named = _train(desc, dims, graphs, labels, prm, stream=(DSEED, STEP))
    _, _, o_g, o_pred = dc.make_oracle(desc, dims, prm, plan, graphs, DSEED, STEP).loss_and_grads(graphs, labels)
    assert set(o_g) == set(prm)
    sc.well_conditioned(labels, o_pred)
    np.testing.assert_allclose(pred.reshape(-1), o_pred, rtol=1e-4, atol=1e-4)
    _assert_grads(named, o_g, "P %d: " % P)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 257])
@pytest.mark.parametrize("output", ["linear", "sigmoid"])
def test_losses_on_engine_predictions(output, P):
    """Engine.loss of every kind whose domain the engine's own P predictions fall in (labels drawn in the
    kind's domain), against tests/keras_restated.py at 1e-5 relative: the four kinds defined everywhere
    always run, and all eight on the sigmoid-output predict network (predictions in (0, 1))."""
    if output == "linear":
        _, _, _, plan, graphs, _, prm = sc.case_inputs("p%d" % P)
    else:
        plan, graphs, prm = _sigmoid_case(P)
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    p = b.forward().reshape(-1).copy()
    b.close()
    assert p.shape == (P,) and np.isfinite(p).all()
    rng = np.random.default_rng(P)
    ran = []
    for kind, name in enumerate(kr.LOSSES):
        if name == "BinaryCrossentropy":
            y, ok = rng.uniform(0.0, 1.0, P).astype(np.float32), bool(np.all((p > 0) & (p < 1)))
        elif name in ("Poisson", "MeanSquaredLogarithmicError", "MeanAbsolutePercentageError"):
            y, ok = rng.uniform(0.05, 3.0, P).astype(np.float32), bool(np.all(p > 0))
        else:
            y, ok = rng.normal(0, 1.5, P).astype(np.float32), True
        if not ok:
            continue
        loss, d = _run_loss(eng, kind, p, y)
        ref = kr.loss(name, p, y)
        print("%s P %d: loss %.12g (float64 %.12g, rel %.3g)" % (name, P, loss, ref, abs(loss - ref) / abs(ref)))
        assert loss == pytest.approx(ref, rel=1e-5)
        assert d.shape == (P,) and np.isfinite(d).all()
        ran.append(name)
    eng.close()
    assert {"MeanSquaredError", "MeanAbsoluteError", "Huber", "LogCosh"} <= set(ran)
    if output == "sigmoid":
        assert ran == kr.LOSSES


@functools.lru_cache(maxsize=None)
def _sigmoid_case(P):
    desc, dims = _t2(predict_model("sigmoid_out", hidden=32)), sc.dims("routenet")
    graphs = [sc.graph(sc.P_GRAPH[P])]
    _, plan, _, prm = sc.inputs_for(desc, dims, graphs)
    return plan, graphs, prm


if __name__ == "__main__":
    _ts_child(sys.argv[1])
