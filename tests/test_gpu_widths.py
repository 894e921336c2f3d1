"""Entities of unequal hidden_state_dimension (message width DIN != destination width H) and entity
features of more than one column (tests/width_cases.py): HIP engine vs the float64 oracles, on two
NSFNET graphs (one case: NSFNET + a synth50 Q-size graph whose nodes carry >= 64 messages), T <= 3.

Forward: predictions and every entity's final state within test_gpu_parity's bound,
|engine - oracle| <= 1e-4 * max(1, |oracle|) (the >= 64-message case: its _ieee_tol rule), and the same
bits per graph, on NaN-poisoned scratch, with int32 indices and from the JSON-lowered plan.
Training: test_gpu_training's _check (every gradient tensor within 1e-4 relative L2 of float64 autograd).

A kernel that takes H where it means DIN (a row stride, a tile count, a pack offset, a scratch size)
passes every test in which all entities share one width; here it cannot."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from ignnition_amd import _lib
from ignnition_amd.engine import Batch, Engine, device_count
from oracle.train_oracle import adam_step
from tests.test_gpu_parity import TOL, _close, _ieee_tol, _narrowed, _run, _scaled_err
from tests.test_gpu_training import _check, _engine_grads
from tests.width_cases import (BIG_SUM, CASES, QSIZE_WIDTHS, RESIDENT, ROUTENET_WIDTHS, case_inputs, reference, BIAS,
                               SEED)

pytestmark = pytest.mark.gpu

ALL = sorted(CASES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _forward(case, graphs=None, json_plan=False, info=None):
    """(predictions, {entity: final states}) of a fresh engine under the current environment, and
    the batch's ign_batch_resident_info into ``info``."""
    desc, dims, _, plan, g, _, prm = case_inputs(case)
    eng = Engine(plan, 0)
    if json_plan:
        h = C.c_void_p()
        _lib.check(_lib.lib.ign_plan_create_json(json.dumps(desc).encode(), json.dumps(dims).encode(), 0, C.byref(h)))
        _lib.lib.ign_plan_destroy(eng.handle)
        eng.handle = h
    eng.set_params(prm)
    b = Batch(eng, g if graphs is None else graphs)
    out = b.forward().reshape(-1).copy()
    states = {e: b.state(e) for e in plan.entities}
    if info is not None:
        info.update(b.resident_info())
    b.close()
    eng.close()
    return out, states


_BASE = {}


def _base(case):
    """The default environment's result, computed once per case and shared by the bitwise tests."""
    if case not in _BASE:
        _BASE[case] = _forward(case)
    return _BASE[case]


def _same_bits(got, exp, what):
    np.testing.assert_array_equal(got[0], exp[0], err_msg="%s: predictions" % what)
    for e in exp[1]:
        np.testing.assert_array_equal(got[1][e], exp[1][e], err_msg="%s: final %s states" % (what, e))


def _tolerance(case):
    if case not in BIG_SUM:
        return TOL
    _, _, _, plan, graphs, _, prm = case_inputs(case)
    return _ieee_tol(plan, graphs, prm, reference(case)[0])


def _check_against_oracle(case, out, states, tol, what=""):
    ref, ref_states = reference(case)
    errs = {"predictions": _scaled_err(out, ref)}
    for e, s in states.items():
        assert s.shape == ref_states[e].shape, e
        errs[e] = _scaled_err(s, ref_states[e])
    print("%s%s: max scaled error vs float64 oracle %s (tolerance %.3g)"
          % (case, what, {k: "%.3g" % v for k, v in errs.items()}, tol))
    _close(out, ref, tol)
    for e, s in states.items():
        _close(s, ref_states[e], tol)


@pytest.mark.parametrize("case", ALL)
def test_forward_matches_oracle(case):
    """Predictions and each entity's final state (at its own width) against the float64 oracle, and the
    path that ran: one graph-resident launch for the resident feature cases, none for any other."""
    desc, dims, _, plan, graphs, _, _ = case_inputs(case)
    ref, _ = reference(case)
    assert np.ptp(ref) > 1e-3, "the oracle's predictions are constant"
    out, ref_run, b, _ = _run(desc, dims, graphs, seed=SEED, bias=BIAS)
    np.testing.assert_array_equal(ref_run, ref)   # _run's oracle: the same parameters as reference()'s
    states = {e: b.state(e) for e in plan.entities}
    for e, h in zip(plan.entities, plan.hidden):
        assert states[e].shape[1] == h
    _check_against_oracle(case, out, states, _tolerance(case))
    eng = b.engine
    eng.set_timing(True)
    again = b.forward()
    st = eng.stats()
    info = b.resident_info()
    b.close()
    eng.close()
    np.testing.assert_array_equal(again, out)
    resident = int(case in RESIDENT)
    print("%s: mp_resident launches %d" % (case, st["mp_resident"]["launches"]))
    assert st["mp_resident"]["launches"] == resident and info["active"] == resident, (st["mp_resident"], info)
    assert (st["seq_gru"]["launches"] == 0) == bool(resident), st["seq_gru"]


@pytest.mark.parametrize("case", ALL)
def test_batch_equals_per_graph(case):
    graphs = case_inputs(case)[4]
    base = _base(case)
    parts = [_forward(case, [g]) for g in graphs]
    _same_bits((np.concatenate([p[0] for p in parts]),
                {e: np.concatenate([p[1][e] for p in parts], axis=0) for e in base[1]}), base, "graph by graph")


@pytest.mark.parametrize("case", ALL)
def test_poisoned_scratch_gives_the_same_bits(monkeypatch, case):
    """IGN_POOL_POISON=1: every scratch block starts as NaN, so a kernel that reads DIN-sized scratch as
    H-sized (or the reverse) shows up as NaN."""
    base = _base(case)
    monkeypatch.setenv("IGN_POOL_POISON", "1")
    _same_bits(_forward(case), base, "IGN_POOL_POISON=1")


@pytest.mark.parametrize("case", ALL)
def test_int32_indices_give_the_same_bits(case):
    _same_bits(_forward(case, _narrowed(case_inputs(case)[4])), _base(case), "int32 indices")


@pytest.mark.parametrize("case", ALL)
def test_json_plan_gives_the_same_bits(case):
    _same_bits(_forward(case, json_plan=True), _base(case), "ign_plan_create_json")


@pytest.mark.parametrize("case", ROUTENET_WIDTHS)
def test_ordered_update_variants(monkeypatch, case):
    """The f32-MFMA ordered update (IGN_SEQ_VARIANT=2) and the default on a table projected from rows of
    another width: both within TOL of the oracle."""
    monkeypatch.setenv("IGN_SEQ_VARIANT", "2")
    out, states = _forward(case)
    _check_against_oracle(case, out, states, TOL, " IGN_SEQ_VARIANT=2")
    monkeypatch.delenv("IGN_SEQ_VARIANT")
    _check_against_oracle(case, *_base(case), TOL, " default")


@pytest.mark.parametrize("case", BIG_SUM)
def test_windowed_and_segmented_sums(monkeypatch, case):
    """A destination of >= 64 messages at DIN 16 into a 32-wide cell: the segmented sum (the default rule,
    and IGN_SUM_WINDOW=2 for every destination) and the windowed sum (IGN_SUM_WINDOW=1)."""
    tol = _tolerance(case)
    graphs = case_inputs(case)[4]
    a = "dst_adj_paths_nodes"
    assert max(np.bincount(np.asarray(g[a])).max() for g in graphs) >= 64
    _check_against_oracle(case, *_base(case), tol, " default")
    for v in ("1", "2"):
        monkeypatch.setenv("IGN_SUM_WINDOW", v)
        out, states = _forward(case)
        _check_against_oracle(case, out, states, tol, " IGN_SUM_WINDOW=" + v)


@pytest.mark.parametrize("case", RESIDENT)
def test_resident_feature_loads(monkeypatch, case):
    """The graph-resident forward loads the features itself (row stride F, zero padding to H): the same
    bits as the batched launches (IGN_RESIDENT=0), with one graph per workgroup and with two."""
    info = {}
    base = _base(case)
    monkeypatch.setenv("IGN_RESIDENT", "0")
    _same_bits(_forward(case, info=info), base, "IGN_RESIDENT=0")
    assert info["active"] == 0
    monkeypatch.delenv("IGN_RESIDENT")
    for k in ("1", "2"):
        monkeypatch.setenv("IGN_RES_GROUP", k)
        got = _forward(case, info=info)
        print("%s IGN_RES_GROUP=%s: %s" % (case, k, {n: info[n] for n in ("active", "form", "workgroups",
                                                                          "graphs_per_workgroup")}))
        assert info["active"] == 1
        if k == "2":
            assert info["graphs_per_workgroup"] in (1, 2)   # 1: two graphs do not fit one workgroup's LDS
        else:
            assert info["graphs_per_workgroup"] == 1
        _same_bits(got, base, "IGN_RES_GROUP=" + k)


# ---------------------------------------------------------------------------------------------
# training
def _flat_grads(case, eng=None):
    desc, dims, _, _, graphs, labels, prm = case_inputs(case)
    eng, b, pred, loss, _, grads = _engine_grads(desc, dims, graphs, labels, prm, eng)
    g = grads.cpu().numpy()
    b.close()
    return eng, pred.reshape(-1), loss, g


@pytest.mark.parametrize("case", ALL)
def test_gradients_match_autograd(case):
    desc, dims, _, _, graphs, labels, prm = case_inputs(case)
    print(case)
    eng, b = _check(desc, dims, graphs, labels, prm)
    b.close()
    eng.close()


@pytest.mark.parametrize("case", ROUTENET_WIDTHS + QSIZE_WIDTHS)
def test_host_built_transposed_csrs(monkeypatch, case):
    """IGN_TRAIN_CSR_GPU=0 (the training tables' transposed CSRs built on the host): the same gradients,
    bitwise, with source rows and steps of different widths."""
    _, _, _, g_gpu = _flat_grads(case)
    monkeypatch.setenv("IGN_TRAIN_CSR_GPU", "0")
    _, _, _, g_host = _flat_grads(case)
    assert np.abs(g_host).sum() > 0
    np.testing.assert_array_equal(g_gpu, g_host)


@pytest.mark.parametrize("case", RESIDENT)
def test_resident_training_forward(monkeypatch, case):
    """The training forward as one graph-resident launch (default) and as per-MP launches
    (IGN_RESIDENT_TRAIN=0), on features of several columns: predictions, loss and gradients bitwise equal."""
    runs = {}
    for v in ("1", "0"):
        monkeypatch.setenv("IGN_RESIDENT_TRAIN", v)
        desc, dims, _, plan, graphs, labels, prm = case_inputs(case)
        eng = Engine(plan, 0)
        eng.set_params(prm)
        eng.set_timing(True)
        eng, pred, loss, g = _flat_grads(case, eng)
        assert eng.stats()["mp_resident"]["launches"] == int(v)
        runs[v] = (pred, loss, g)
        eng.close()
    np.testing.assert_array_equal(runs["1"][0], runs["0"][0])
    assert runs["1"][1] == runs["0"][1]
    np.testing.assert_array_equal(runs["1"][2], runs["0"][2])


def test_adam_step_and_repacked_fragments():
    """One Adam step on rn_l16_p32 against the float64 Keras restatement, then a forward on the repacked
    fragments (W [16][96] and [32][48]) bitwise equal to a fresh plan's with the same parameters."""
    desc, dims, _, plan, graphs, labels, prm = case_inputs("rn_l16_p32")
    eng, b, pred, loss, g, grads = _engine_grads(desc, dims, graphs, labels, prm)
    m = torch.zeros_like(grads)
    v = torch.zeros_like(grads)
    ref = {k: np.asarray(x, np.float64) for k, x in prm.items()}
    rm = {k: np.zeros_like(x) for k, x in ref.items()}
    rv = {k: np.zeros_like(x) for k, x in ref.items()}
    eng.adam_step(grads, m, v, 0, 0.01)
    adam_step(ref, {k: g[k].astype(np.float64) for k in ref}, rm, rv, 0, 0.01)
    got = eng.get_params()
    for k in ref:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-5, atol=1e-6)
    fresh = Engine(plan, 0)
    fresh.set_params(got)
    np.testing.assert_array_equal(Batch(fresh, graphs).forward(), Batch(eng, graphs).forward())
