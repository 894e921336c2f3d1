"""GRU cell options on the CPU (no GPU): activation, recurrent_activation, use_bias and reset_after of a
recurrent update (tests/gru_cases.py) through both front ends -- Model_information -> MPPlan ->
ign_plan_create + ign_plan_set_cell_options, and ign_plan_create_json -- give the same plan; the
parameter table carries the [3H] bias or none; the defaults written out are the plan of absent keys;
every other GRUCell key and every activation outside the ten lowered names is refused with the same text
from both; the options are final once a batch exists; plan_lower.cpp takes a cell with options off the
resident, split and fused paths (tests/cpp/cell_options_check.cpp); and the oracle subclasses restate the
parents' default cell to the bit."""
import copy
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ignnition_amd import _lib, model_examples, synthetic, workloads
from ignnition_amd.engine import MPPlan, UnsupportedModel
from ignnition_amd.json_operations import Model_information
from oracle.dense_forward import DenseOracle
from oracle.train_oracle import TorchOracle
from tests import gru_cases as gc
from tests.test_plan_json import ROUTENET_DIMS, _create_json, _describe, _tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _python_plan(desc, dims):
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    d, keep = plan.to_desc()
    h = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create(C.byref(d), 0, C.byref(h)))
    plan.set_cell_options(h)
    return plan, h


def _cells(plan):
    """An MPPlan's cells in the layout of ign_plan_describe_json's "cells"."""
    return [{"name": n, "input_dim": din, "units": h, "activation": a, "recurrent_activation": r, "use_bias": b,
             "reset_after": ra} for (n, din, h), (a, r, b, ra) in zip(plan.cells, plan.cell_options)]


@pytest.mark.parametrize("case", sorted(gc.CASES))
def test_both_front_ends_lower_the_same_plan(case):
    """On the parent commit the first case raises UnsupportedModel ("GRU options [...] are not lowered")."""
    desc, dims, _ = gc.CASES[case]()
    plan, hp = _python_plan(desc, dims)
    rc, hj = _create_json(desc, dims)
    try:
        assert rc == 0, _lib.lib.ign_last_error()
        assert _tensors(hj) == _tensors(hp)
        info = _describe(hj)
        specs = plan.param_specs()
        assert [p["name"] for p in info["params"]] == [n for n, _ in specs]
        assert [tuple(p["shape"]) for p in info["params"]] == [tuple(s) for _, s in specs]
        assert info["cells"] == _cells(plan)
        assert any(c != _cells_default(c) for c in info["cells"]), "the case has no cell with options"
    finally:
        _lib.lib.ign_plan_destroy(hp)
        if hj:
            _lib.lib.ign_plan_destroy(hj)


def _cells_default(c):
    return dict(c, activation=_lib.ACT["tanh"], recurrent_activation=_lib.ACT["sigmoid"], use_bias=True, reset_after=True)


def test_bias_tensor_forms():
    """[2][3H] by default, [3H] under reset_after false, none under use_bias false: in the names, in the
    engine's tensor table (kind 2) and in init_params."""
    for case, link, path in (("rn_v1", (96,), (96,)), ("rn_no_bias", None, None), ("rn_relu", (2, 96), (2, 96)),
                             ("rn_all_four", None, None), ("rn_v1_l16_p32", (48,), (96,)),
                             ("rn_v1_h64", (192,), (192,)), ("qs_path_v1", (2, 96), (96,))):
        desc, dims, _ = gc.CASES[case]()
        plan, h = _python_plan(desc, dims)
        try:
            specs = dict(plan.param_specs())
            assert specs.get("link_update/bias") == link and specs.get("path_update/bias") == path, case
            bias = [(r, c) for k, _, _, r, c in _tensors(h)[0] if k == 2]
            want = [s if len(s) == 2 else (1,) + s for s in (specs.get(n + "_update/bias") for n, _, _ in plan.cells) if s]
            assert bias == want, case
            prm = plan.init_params(0, bias_scale=0.1)
            assert set(prm) == set(specs) and all(prm[n].shape == tuple(s) for n, s in specs.items())
        finally:
            _lib.lib.ign_plan_destroy(h)


@pytest.mark.parametrize("model", sorted(gc.DEFAULTS_WRITTEN))
def test_written_out_defaults_are_the_default_plan(model):
    absent, written = (b() for b in gc.DEFAULTS_WRITTEN[model])
    assert absent[0] != written[0]
    docs, tensors = [], []
    for desc, dims, _ in (absent, written):
        plan, hp = _python_plan(desc, dims)
        rc, hj = _create_json(desc, dims)
        try:
            assert rc == 0, _lib.lib.ign_last_error()
            assert _tensors(hj) == _tensors(hp)
            tensors.append(_tensors(hj))
            docs.append(json.dumps(_describe(hj), sort_keys=True))
        finally:
            _lib.lib.ign_plan_destroy(hp)
            _lib.lib.ign_plan_destroy(hj)
    assert tensors[0] == tensors[1] and docs[0] == docs[1]


@pytest.mark.parametrize("keys,text", [
    ({"dropout": 0.1}, "GRU options ['dropout'] are not lowered (Keras defaults only)"),
    ({"recurrent_dropout": 0.1, "reset_after": False}, "GRU options ['recurrent_dropout'] are not lowered (Keras defaults only)"),
    ({"kernel_initializer": "zeros", "implementation": 1, "use_bias": False},
     "GRU options ['implementation', 'kernel_initializer'] are not lowered (Keras defaults only)"),
    ({"activation": "swish"}, "activation 'swish' not supported"),
    ({"recurrent_activation": "softmax"}, "activation 'softmax' not supported"),
    ({"activation": "SELU"}, "activation 'SELU' not supported"),
])
def test_refusals_have_one_text(keys, text):
    """Only the keys that are not lowered are listed; a lowered key beside them is not."""
    desc = model_examples.routenet(iterations=2)
    gc._gru(desc).update(keys)
    with pytest.raises(UnsupportedModel) as e:
        MPPlan.from_model_info(Model_information(copy.deepcopy(desc), ROUTENET_DIMS))
    assert str(e.value) == text
    rc, h = _create_json(desc, ROUTENET_DIMS)
    if h:
        _lib.lib.ign_plan_destroy(h)
    assert rc == -2 and _lib.lib.ign_last_error().decode() == text


def test_activation_that_is_no_string_is_invalid_from_both():
    """A list or dict as the activation: ValueError / IGN_ERR_INVALID with one text, not a TypeError."""
    for key, value in (("activation", ["relu"]), ("recurrent_activation", {"name": "sigmoid"})):
        desc = model_examples.routenet(iterations=2)
        gc._gru(desc)[key] = value
        text = "GRU %s: expected a string" % key
        with pytest.raises(ValueError) as e:
            MPPlan.from_model_info(Model_information(copy.deepcopy(desc), ROUTENET_DIMS))
        assert str(e.value) == text
        rc, h = _create_json(desc, ROUTENET_DIMS)
        if h:
            _lib.lib.ign_plan_destroy(h)
        assert rc == -1 and _lib.lib.ign_last_error().decode() == text


def test_set_cell_options_arguments_and_order():
    """IGN_ERR_INVALID (-1) for a bad cell index or activation code, and once a batch of the plan was asked
    for: parameter and training buffers are sized from the options."""
    plan = MPPlan.from_model_info(Model_information(model_examples.routenet(iterations=2), ROUTENET_DIMS))
    d, keep = plan.to_desc()
    h = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create(C.byref(d), 0, C.byref(h)))
    try:
        call = _lib.lib.ign_plan_set_cell_options
        opt = lambda *v: C.byref(_lib.CellOptions(*v))
        before = _tensors(h)
        assert call(h, 2, opt(4, 3, 1, 1)) == -1 and b"cell 2 outside 0..1" in _lib.lib.ign_last_error()
        assert call(h, 0, opt(10, 3, 1, 1)) == -1 and b"activation code 10" in _lib.lib.ign_last_error()
        assert call(h, 0, opt(4, -1, 1, 1)) == -1
        assert call(h, 0, None) == -1
        assert _tensors(h) == before
        assert call(h, 0, opt(4, 3, 1, 0)) == 0
        v1 = _tensors(h)
        assert v1 != before and [(o, r, c) for k, o, _, r, c in v1[0] if k == 2] == [(0, 1, 96), (1, 2, 96)]
        assert call(h, 0, opt(4, 3, 0, 1)) == 0
        assert [(o, r, c) for k, o, _, r, c in _tensors(h)[0] if k == 2] == [(1, 2, 96)]
        assert call(h, 0, opt(4, 3, 1, 1)) == 0 and _tensors(h) == before
        out = C.c_void_p()
        assert _lib.lib.ign_batch_create(h, C.byref(_lib.BatchDesc()), C.byref(out)) != 0   # (no graphs: refused)
        assert call(h, 0, opt(4, 3, 0, 1)) == -1
        assert b"ign_plan_set_cell_options after a batch of the plan was created" in _lib.lib.ign_last_error()
        assert _tensors(h) == before
    finally:
        _lib.lib.ign_plan_destroy(h)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_cell_options_check(tmp_path, flags):
    """plan_lower.cpp's set_cell_options as a stand-alone program: a cell with options loses the fragments
    the resident forward, the split variants and the fused paths need."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the lowering check"
    exe = str(tmp_path / "cell_options_check")
    src = [os.path.join(ROOT, "tests", "cpp", "cell_options_check.cpp"),
           os.path.join(ROOT, "ignnition_amd", "csrc", "plan_lower.cpp")]
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", *flags, *src, "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]


def test_oracle_subclasses_restate_the_default_cell_to_the_bit():
    """RouteNet on NSFNET with default options: CellDenseOracle / CellTorchOracle equal their parents in
    predictions, final states, loss and every gradient, to the last bit."""
    desc = model_examples.routenet(iterations=2)
    mi = Model_information(copy.deepcopy(desc), ROUTENET_DIMS)
    graphs, labels = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", g) for g in range(2)])
    prm = MPPlan.from_model_info(mi).init_params(gc.SEED, bias_scale=gc.BIAS)
    for dtype in (np.float64, np.float32):
        a, b = DenseOracle(desc, ROUTENET_DIMS, prm, dtype=dtype), gc.CellDenseOracle(desc, ROUTENET_DIMS, prm, dtype=dtype)
        np.testing.assert_array_equal(a.forward(graphs), b.forward(graphs))
        sa, sb = a.final_states(graphs[0]), b.final_states(graphs[0])
        for e in sa:
            np.testing.assert_array_equal(sa[e], sb[e])
    la, ra, ga, pa = TorchOracle(desc, ROUTENET_DIMS, prm).loss_and_grads(graphs, labels)
    lb, rb, gb, pb = gc.CellTorchOracle(desc, ROUTENET_DIMS, prm).loss_and_grads(graphs, labels)
    assert la == lb and ra == rb
    np.testing.assert_array_equal(pa, pb)
    assert set(ga) == set(gb)
    for k in ga:
        np.testing.assert_array_equal(ga[k], gb[k])


def test_oracle_restatement_against_finite_differences():
    """The torch restatement's gradients of the all-four cell against central differences of the numpy one
    (float64), on one step of random rows: the two restatements are one function."""
    import torch
    rng = np.random.default_rng(3)
    H, D, N = 8, 5, 6
    o = dict(gc.GRU_OPTION_DEFAULTS, **dict(gc.ALL_FOUR, activation="tanh"))   # (smooth: finite differences across relu's kink prove nothing)
    x, h = rng.normal(size=(N, D)), rng.normal(size=(N, H))
    k, rk = rng.normal(size=(D, 3 * H)) * 0.5, rng.normal(size=(H, 3 * H)) * 0.5
    for bias in (None, rng.normal(size=(3 * H,)) * 0.3):
        t = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, h, k, rk)]
        tb = None if bias is None else torch.tensor(bias, dtype=torch.float64)
        gc.gru_cell_torch(t[0], t[1], t[2], t[3], tb, o).sum().backward()
        f = lambda rk_: gc.gru_cell_np(x, h, k, rk_, bias, o).sum()
        num = np.zeros_like(rk)
        for i in range(H):
            for j in range(3 * H):
                e = np.zeros_like(rk)
                e[i, j] = 1e-6
                num[i, j] = (f(rk + e) - f(rk - e)) / 2e-6
        np.testing.assert_allclose(t[3].grad.numpy(), num, rtol=1e-6, atol=1e-8)
