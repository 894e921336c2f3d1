"""The predict network beyond 256-selu-256-selu-1 (tests/predict_cases.py): HIP engine vs the float64
oracle (oracle/dense_forward.py) on two NSFNET graphs (364 path rows), T = 3.

Tolerance: test_gpu_parity's, |engine - oracle| <= 1e-4 * max(1, |oracle|); the saturating cases use
its IEEE-float32 yardstick rule (_ieee_tol).  Every case's oracle output is checked not to be
degenerate first, so a kernel that returned a constant could not pass."""
import numpy as np
import pytest

from ignnition_amd.engine import Batch, Engine, device_count
from oracle.dense_forward import DenseOracle
from tests.predict_cases import (FUSED, PREDICT_CASES, SATURATED, UNFUSED, forward_case, layer1_activations,
                                 predict_inputs)
from tests.readout_cases import _POOL
from tests.test_gpu_parity import TOL, _close, _ieee_tol, _scaled_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _not_degenerate(case, ref):
    assert np.ptp(ref) > 1e-3, "%s: the oracle's predictions are constant" % case
    if case == "relu_out":
        assert (ref > 0).mean() >= 0.25, "relu_out: %.2f of the oracle's outputs positive" % (ref > 0).mean()


def _forward_twice(plan, prm, graphs, launches):
    """(predictions, flat) of a fresh engine: a second forward of the same batch gives the same bits,
    and the predict network ran as ``launches`` readout launches."""
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    eng.set_timing(True)
    out = b.forward()
    assert eng.stats()["readout"]["launches"] == launches
    eng.set_timing(False)
    again = b.forward()
    b.close()
    eng.close()
    assert np.array_equal(out, again)
    return out


@pytest.mark.parametrize("hidden", [16, 32, 64])
@pytest.mark.parametrize("case", FUSED)
def test_fused_predict_activations(monkeypatch, case, hidden):
    """readout3 (variant 1; every variant at H = 16), readout_bf (2), readout_h16 (4) and readout_h32 (5)
    at each hidden / output activation and without an output bias: one launch, within TOL of the float64
    oracle, bitwise repeatable, and the split-contraction variants within 4x of the f32-MFMA kernel's
    error (or 1e-6), test_split_bf16_contractions_are_fp32_accurate's relation."""
    desc, dims, plan, graphs, _, prm, ref = forward_case(case, hidden)
    assert ref.size == 364
    _not_degenerate(case, ref)
    outs, errs = {}, {}
    for v in ("1", "2", "4", "5"):
        monkeypatch.setenv("IGN_READOUT_VARIANT", v)
        outs[v] = _forward_twice(plan, prm, graphs, 1).reshape(-1)
        errs[v] = _scaled_err(outs[v], ref)
    print("%s H %d: max scaled error vs float64 oracle per readout variant: %s" % (case, hidden, errs))
    for v in outs:
        _close(outs[v], ref)
    if hidden == 16:   # no split-contraction kernel at DIN 16: readout3 whatever the variant
        for v in ("2", "4", "5"):
            assert np.array_equal(outs[v], outs["1"]), v
    else:
        assert not np.array_equal(outs["1"], outs["4"])   # the switch took effect
    for v, e in errs.items():
        assert e <= max(4 * errs["1"], 1e-6), errs


@pytest.mark.parametrize("case", UNFUSED)
def test_unfused_predict_networks(case):
    """Predict networks the fused kernels refuse (act1 != act2, a hidden layer without bias, 1 / 2 / 4
    layers, widths that are no multiple of 4, three output units): one dense_generic launch per layer."""
    desc, dims, plan, graphs, _, prm, ref = forward_case(case, 32)
    _not_degenerate(case, ref)
    layers = PREDICT_CASES[case]
    out = _forward_twice(plan, prm, graphs, len(layers))
    assert out.shape == (364, layers[-1][0])
    if case == "out3":   # row-major [P][3]: path p's three outputs are consecutive, as the oracle's reshape(-1)
        per_graph = np.concatenate([DenseOracle(desc, dims, prm).forward_graph(g) for g in graphs], axis=0)
        assert per_graph.shape == (364, 3)
        assert np.ptp(per_graph, axis=0).min() > 1e-3 and np.abs(per_graph[:, 0] - per_graph[:, 1]).max() > 1e-2
        _close(out[:, 1], per_graph[:, 1])
        np.testing.assert_array_equal(per_graph.reshape(-1), ref)
    _close(out, ref)


@pytest.mark.parametrize("hidden", [32, 64])
@pytest.mark.parametrize("case", sorted(SATURATED))
def test_saturating_predict_networks(monkeypatch, case, hidden):
    """Layers 1 and 2 (kernel and bias) scaled by SATURATED[case] (x16; x64 for tanh and sigmoid, where
    x16 leaves under 30 % of the layer-1 activations at an asymptote): relu's and selu's layer-2 inputs
    reach the hundreds (the fp16 scale bound A mx + B of variant 4), selu's negative arm sits at
    -lambda alpha, tanh and sigmoid saturate.  Variants 1 and 4 stay finite and within the IEEE-float32
    yardstick of the float64 oracle."""
    desc, dims, plan, graphs, _, prm, ref = forward_case(case, hidden)
    _not_degenerate(case, ref)
    if case in ("sat_tanh", "sat_sigmoid"):
        a = layer1_activations(case, hidden)
        sat = np.abs(a) > 1 - 1e-3 if case == "sat_tanh" else (a < 1e-3) | (a > 1 - 1e-3)
        assert sat.mean() >= 0.5, "%s: %.2f of the layer-1 activations saturated" % (case, sat.mean())
    tol = _ieee_tol(plan, graphs, prm, ref)
    errs = {}
    for v in ("1", "4"):
        monkeypatch.setenv("IGN_READOUT_VARIANT", v)
        out = _forward_twice(plan, prm, graphs, 1).reshape(-1)
        assert np.all(np.isfinite(out))
        errs[v] = _scaled_err(out, ref)
    print("%s H %d: max scaled error vs float64 oracle per readout variant: %s (tolerance %.3g)"
          % (case, hidden, errs, tol))
    for v, e in errs.items():
        assert e <= tol, errs


@pytest.mark.parametrize("case", ["four_layer", "mixed", "nobias_hidden", "linear"])
def test_json_lowered_predict_network(case):
    """The C++ lowering of model_description.json (ign_plan_create_json) reads the predict network's
    activation strings and use_bias as the Python lowering does: bitwise-equal predictions, themselves
    within TOL of the oracle.  (tests/test_plan_json.py compares the parameter tensors only.)"""
    import ctypes as C
    import json

    from ignnition_amd import _lib
    desc, dims, plan, graphs, _, prm, ref = forward_case(case, 32)
    e1 = Engine(plan, 0)
    e1.set_params(prm)
    out = Batch(e1, graphs).forward()
    _close(out, ref)
    e2 = Engine(plan, 0)
    h = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create_json(json.dumps(desc).encode(), json.dumps(dims).encode(), 0, C.byref(h)))
    _lib.lib.ign_plan_destroy(e2.handle)
    e2.handle = h
    e2.set_params(prm)
    np.testing.assert_array_equal(Batch(e2, graphs).forward(), out)


@pytest.mark.parametrize("case", ["relu", "tanh"])
def test_fused_predict_on_three_rows(monkeypatch, case):
    """Predict on a pooled graph tensor of three graphs (P = 3): the fused kernels' non-selu arms on a
    row tile whose other 13 (or 29) rows are out of range."""
    pool = [_POOL("sum", "path", "g")]
    desc, dims, plan, graphs, _, prm = predict_inputs(case, 32, n_graphs=3, ops=pool, predict_input=["g"])
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    assert ref.size == 3
    _not_degenerate(case, ref)
    for v in ("1", "2", "4", "5"):
        monkeypatch.setenv("IGN_READOUT_VARIANT", v)
        _close(_forward_twice(plan, prm, graphs, 1), ref)
