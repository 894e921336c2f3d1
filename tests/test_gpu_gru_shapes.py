"""The table of tests/gru_shape_cases.py on the GPU: GRU cells with options (gru_cell.hip's seq_gru_cell,
sum_gru_cell and their backward kernels) on graphs whose path, link, node and message counts sit on those
kernels' row-tile, step, in-degree and block edges, and on mp_step.cpp's pre-summed route, which a plan
with an option cell takes for rows of >= 64 messages in the training forward too.

Every check is an existing helper with its own bound: test_gpu_gru_options' rule max(TOL, 4 x the float32
numpy run's error) through test_gpu_parity's _close (tests/test_gru_shape_cases.py holds 4 x that error
below TOL on every entry, so TOL is the bound of every entry), test_gpu_training's _check_grads (GTOL per
tensor, loss and l2 at 1e-5), the Adam step of test_gpu_gru_options and test_gpu_input_gradients'
_check_case.  Each test prints the engine's error beside the float32 yardstick."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ignnition_amd.engine import Batch, Engine, device_count
from oracle.train_oracle import adam_step
from tests import gru_shape_cases as gs
from tests.input_grad_oracle import CellInputGradOracle
from tests.test_gpu_dropout import _assert_grads
from tests.test_gpu_input_gradients import _check_case
from tests.test_gpu_parity import TOL, _close, _scaled_err
from tests.test_gpu_training import _check_grads, _engine_grads

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(gs.CASES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _set_env(monkeypatch, name):
    for k, v in gs.CASES[name][0].env:
        monkeypatch.setenv(k, v)


def _tolerance(name):
    """test_gpu_gru_options._tolerance on an entry of this table."""
    f32 = gs.float32_error(name)
    print("%s: float32 numpy run vs float64: max scaled error %.3g -> tolerance %.3g" % (name, f32, max(TOL, 4 * f32)))
    return max(TOL, 4 * f32)


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
def test_forward_matches_oracle(monkeypatch, name):
    """Predictions and every entity's final states against CellDenseOracle (float64); no graph-resident
    launch; a second forward and, after enable_training, forward_train give the same bits (on an entry
    with a row of >= 64 messages or the windowed sum, through launch_sum_seg / launch_sum_win and the
    identity CSR in both).

    Measured on the MI355X: the engine's error is 7.5e-8 .. 3.8e-6 (largest: p257/ALL_FOUR) against float32
    yardsticks of 9.8e-8 .. 1.6e-5.  What this test found: at a path width of 16 (h16_deg64/V1, h16_p17/V1,
    h16_p17/HS_NO_BIAS; in-degree 10 as well as 64) forward_train was up to 2.8e-7 away from forward.  The
    cause was the readout, not a cell: a predict input of 16 columns has no split-bf16 pieces, so ign_forward
    runs the fused f32 readout3_kernel, which had no saving form, and ign_forward_train_end ran the same
    stack layer by layer.  readout3_kernel now has a saving form, and the training forward of a plan with an
    option cell takes it wherever readout3 is the inference readout."""
    _set_env(monkeypatch, name)
    _, _, _, plan, graphs, _, prm = gs.case_inputs(name)
    ref, ref_states = gs.reference(name)
    tol = _tolerance(name)
    eng = Engine(plan, 0)
    eng.set_params(prm)
    eng.set_timing(True)
    b = Batch(eng, graphs)
    out = b.forward().reshape(-1).copy()
    states = {e: b.state(e) for e in plan.entities}
    st, info = eng.stats(), b.resident_info()
    errs = dict({e: _scaled_err(s, ref_states[e]) for e, s in states.items()}, predictions=_scaled_err(out, ref))
    print("%s: max scaled error vs float64 oracle %.3g %s (tolerance %.3g, max in-degree %d)"
          % (name, max(errs.values()), {k: "%.3g" % v for k, v in errs.items()}, tol, gs.max_in_degree(name)))
    _close(out, ref, tol)
    for e, s in states.items():
        assert s.shape == ref_states[e].shape
        _close(s, ref_states[e], tol)
    assert info["active"] == 0 and st["mp_resident"]["launches"] == 0, (info, st["mp_resident"])
    assert st["seq_gru"]["launches"] > 0
    np.testing.assert_array_equal(b.forward().reshape(-1), out, err_msg="the second forward")
    b.enable_training()
    np.testing.assert_array_equal(b.forward_train().reshape(-1), out, err_msg="forward_train")
    b.close()
    eng.close()


@pytest.mark.parametrize("name", ALL)
def test_placement_and_poisoned_scratch(monkeypatch, name):
    """test_gpu_shapes' test of the same name on this table: each graph's predictions are the same bits
    alone and at every rotation of its batch, and the entry's are the same bits on NaN-poisoned scratch
    (IGN_POOL_POISON=1); the default run is within the tolerance of the cached float64 oracle."""
    _set_env(monkeypatch, name)
    _, _, _, plan, graphs, _, prm = gs.case_inputs(name)
    ref = gs.reference(name)[0]
    n = len(graphs)
    rotations = [graphs[r:] + graphs[:r] for r in range(n)]
    outs = _predictions(plan, prm, rotations + [[g] for g in graphs])
    whole, alone = outs[0], outs[n:]
    print("%s: max scaled error vs float64 oracle %.3g" % (name, _scaled_err(whole, ref)))
    _close(whole, ref, _tolerance(name))
    np.testing.assert_array_equal(whole, np.concatenate(alone))
    for r in range(1, n):
        np.testing.assert_array_equal(outs[r], np.concatenate(alone[r:] + alone[:r]), err_msg="rotation %d" % r)
    monkeypatch.setenv("IGN_POOL_POISON", "1")
    np.testing.assert_array_equal(_predictions(plan, prm, [graphs])[0], whole)


@pytest.mark.parametrize("name", ALL)
def test_gradients(monkeypatch, name):
    """_check_grads against CellTorchOracle's float64 autograd (one tensor per parameter: no bias entry
    under use_bias false), then the same gradient bits with host-built transposed CSRs
    (IGN_TRAIN_CSR_GPU=0) and on NaN-poisoned scratch (IGN_POOL_POISON=1, a fresh engine and batch: a
    gu / gu2 / rh row that no lane wrote would reach a contraction as NaN).

    IGN_RESIDENT_TRAIN=0 is left out: the resident training forward needs resident_plan_shape, which
    refuses a plan whose ordered cell has no split-fp16 pieces (pk_uh), and a Q-size plan whose path cell
    alone has options fails the same test; the knob selects nothing for these plans."""
    _set_env(monkeypatch, name)
    desc, dims, _, plan, graphs, labels, prm = gs.case_inputs(name)
    print(name)
    oracle = gs.autograd(name)
    assert set(oracle[2]) == set(prm) == {n for n, _ in plan.param_specs()}
    eng, b, grads = _check_grads(desc, dims, graphs, labels, prm, oracle=oracle)
    base = grads.cpu().numpy()
    b.close()
    eng.close()
    assert np.isfinite(base).all() and np.abs(base).sum() > 0
    for switch, value in (("IGN_TRAIN_CSR_GPU", "0"), ("IGN_POOL_POISON", "1")):
        with monkeypatch.context() as m:
            m.setenv(switch, value)
            eng, b, _, _, _, g = _engine_grads(desc, dims, graphs, labels, prm)
            got = g.cpu().numpy()
            b.close()
            eng.close()
        np.testing.assert_array_equal(got, base, err_msg="%s=%s" % (switch, value))


# ---------------------------------------------------------------------------------------------
# ts_plan's chunks: IGN_TS_MIN_ROWS is read once per process, so one child process runs the entries
def _ts_child(out_path):
    res = {}
    for name in gs.TS_CASES:
        desc, dims, _, _, graphs, labels, prm = gs.case_inputs(name)
        eng, b, pred, loss, _, grads = _engine_grads(desc, dims, graphs, labels, prm)
        res[name + "|grads"], res[name + "|pred"], res[name + "|loss"] = grads.cpu().numpy(), pred.reshape(-1), np.float64(loss)
        b.close()
        eng.close()
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def ts32(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gru_ts32") / "grads.npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.test_gpu_gru_shapes", out]
    run = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, IGN_TS_MIN_ROWS="32"), capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    return dict(np.load(out))


@pytest.mark.parametrize("name", gs.TS_CASES)
def test_gradients_with_32_row_chunks(ts32, name):
    """IGN_TS_MIN_ROWS=32: the row contractions of a reset_after false cell (hs^T gu and rh^T gu2 over
    the saved rows with each sequence's final-state row, x^T ga over the paths) split into chunks of 32
    rows with a short last one.  Every tensor within GTOL of float64 autograd, the loss at 1e-5; over the
    entries the chunking changes at least one gradient bit (the knob reached the child process)."""
    desc, dims, _, plan, graphs, labels, prm = gs.case_inputs(name)
    o_loss, _, o_g, o_pred = gs.autograd(name)
    eng = Engine(plan, 0)
    layout = eng.layout
    eng.close()
    g = ts32[name + "|grads"]
    named = {n: g[off:off + int(np.prod(shape))].reshape(shape) for n, shape, off in layout}
    assert set(named) == set(o_g)
    np.testing.assert_allclose(ts32[name + "|pred"], o_pred, rtol=1e-4, atol=1e-4)
    assert float(ts32[name + "|loss"]) == pytest.approx(o_loss, rel=1e-5)
    _assert_grads(named, o_g, name + " IGN_TS_MIN_ROWS=32: ")
    if name == gs.TS_CASES[-1]:
        differs = []
        for c in gs.TS_CASES:
            d, dm, _, _, gr, lb, pr = gs.case_inputs(c)
            eng, b, _, _, _, base = _engine_grads(d, dm, gr, lb, pr)
            differs.append(not np.array_equal(base.cpu().numpy(), ts32[c + "|grads"]))
            b.close()
            eng.close()
        print("gradient bits differ from the default chunks:", dict(zip(gs.TS_CASES, differs)))
        assert any(differs)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gs.ADAM_CASES)
def test_adam_step(monkeypatch, name):
    """One Adam step from the engine's gradients against the float64 Keras restatement, as
    test_gpu_gru_options takes it."""
    _set_env(monkeypatch, name)
    desc, dims, _, _, graphs, labels, prm = gs.case_inputs(name)
    eng, b, _, _, _, grads = _engine_grads(desc, dims, graphs, labels, prm)
    m, v = torch.zeros_like(grads), torch.zeros_like(grads)
    ref = {k: np.asarray(x, np.float64) for k, x in prm.items()}
    rm = {k: np.zeros_like(x) for k, x in ref.items()}
    rv = {k: np.zeros_like(x) for k, x in ref.items()}
    g = grads.cpu().numpy()
    assert np.isfinite(g).all() and np.abs(g).sum() > 0
    named = {n: g[off:off + int(np.prod(shape))].reshape(shape).astype(np.float64) for n, shape, off in eng.layout}
    eng.adam_step(grads, m, v, 0, 0.01)
    adam_step(ref, named, rm, rv, 0, 0.01)
    got = eng.get_params()
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape
        assert not np.array_equal(got[k], prm[k]), k + " did not move"
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-5, atol=1e-6)
    b.close()
    eng.close()


@pytest.mark.parametrize("name", gs.FEATURE_GRAD_CASES)
def test_feature_gradients(monkeypatch, name):
    """The gradient with respect to the link and path features through the option kernels' backward
    (on deg64 through the pre-summed training forward), against autograd with the columns as leaves."""
    _set_env(monkeypatch, name)
    desc, dims, _, _, graphs, labels, prm = gs.case_inputs(name)
    print(name)
    _check_case(desc, dims, graphs, labels, prm, oracle=CellInputGradOracle)


if __name__ == "__main__":
    _ts_child(sys.argv[1])
