"""The table of tests/resident_cases.py on the GPU: graphs on the resident forward's LDS budget and on the
switches between its forms, the grouped workgroup and the batched fallback.

ign_batch_resident_info is held to the table's restatement first (active, form, lds_bytes,
graphs_per_workgroup, workgroups), so a case on the wrong side of an edge fails before any number is
compared.  Every numeric check is an existing helper with its own bound: test_gpu_parity's
_resident_vs_batched and _close (TOL) and test_gpu_training's _check_grads (GTOL per tensor, loss and l2 at
1e-5)."""
import numpy as np
import pytest

from ignnition_amd.engine import Batch, Engine, device_count
from tests import resident_cases as rc
from tests import shape_cases as sc
from tests.test_gpu_parity import _close, _resident_vs_batched, _scaled_err
from tests.test_gpu_training import _check_grads, _engine_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _set_group(monkeypatch, group):
    if group:
        monkeypatch.setenv("IGN_RES_GROUP", str(group))


def _probe(plan, prm, graphs):
    """resident_info of a fresh batch under the current environment."""
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    info = b.resident_info()
    b.close()
    eng.close()
    return info


def _assert_info(name, info, exp):
    got = {k: info[k] for k in rc.FIELDS}
    print("%s: resident_info %s" % (name, got))
    if exp["active"]:
        assert got == {k: exp[k] for k in rc.FIELDS}, (got, exp)
    else:
        assert got["active"] == 0, got


def _predictions(plan, prm, batches):
    eng = Engine(plan, 0)
    eng.set_params(prm)
    outs = []
    for graphs in batches:
        b = Batch(eng, graphs)
        outs.append(b.forward().reshape(-1).copy())
        b.close()
    eng.close()
    return outs


def _forward_case(monkeypatch, name, exp):
    desc, dims, mi, plan, graphs, _, prm = rc.case_inputs(name)
    monkeypatch.setenv("IGN_RESIDENT", "1")
    _assert_info(name, _probe(plan, prm, graphs), exp)
    info = _resident_vs_batched(monkeypatch, desc, dims, mi, graphs, seed=sc.SEED, bias=sc.BIAS, resident=bool(exp["active"]))
    _assert_info(name, info, exp)
    monkeypatch.setenv("IGN_RESIDENT", "1")   # (_resident_vs_batched leaves it at 0)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_forward_at_the_edge(monkeypatch, name):
    """resident_info as restated; _resident_vs_batched (predictions and final states bitwise the batched
    launches, TOL against the float64 oracle, the launch counts of the route the table expects, hipGraph
    replay bitwise); each graph of a batch entry the same bits alone."""
    c = rc.case(name)
    _set_group(monkeypatch, c.group)
    exp = rc.case_expected(name)
    _forward_case(monkeypatch, name, exp)
    _, _, _, plan, graphs, _, prm = rc.case_inputs(name)
    outs = _predictions(plan, prm, [graphs] + ([[g] for g in graphs] if len(graphs) > 1 else []))
    print("%s: max scaled error vs float64 oracle %.3g" % (name, _scaled_err(outs[0], rc.reference(name))))
    _close(outs[0], rc.reference(name))
    if len(graphs) > 1:
        np.testing.assert_array_equal(outs[0], np.concatenate(outs[1:]))


def test_16bit_rows_of_a_group(monkeypatch):
    """IGN_RES_GROUP=2: 32 768 + 32 767 paths are 65 535 local rows, the last 16-bit one, and run resident;
    one path more and the batch takes the batched launches."""
    monkeypatch.setenv("IGN_RES_GROUP", "2")
    for name in sorted(rc.ROWS16):
        exp = rc.case_expected(name)
        assert exp["active"] == int(name == "d_16bit_fit")
        _forward_case(monkeypatch, name, exp)


@pytest.mark.parametrize("name", sorted(n for n, c in rc.CASES.items() if c.poison))
def test_exact_fit_on_poisoned_scratch(monkeypatch, name):
    """The exact-fit entries on NaN-poisoned pool blocks (IGN_POOL_POISON=1): the same bits."""
    _, _, _, plan, graphs, _, prm = rc.case_inputs(name)
    (base,) = _predictions(plan, prm, [graphs])
    monkeypatch.setenv("IGN_POOL_POISON", "1")
    _assert_info(name, _probe(plan, prm, graphs), rc.case_expected(name))
    np.testing.assert_array_equal(_predictions(plan, prm, [graphs])[0], base)
    _close(base, rc.reference(name))


# ---------------------------------------------------------------------------------------------
# F. the shape table under the other forms
@pytest.mark.parametrize("name", rc.PG_SHAPES)
def test_shapes_in_the_path_global_form(monkeypatch, name):
    """Every H = 32 entry of tests/shape_cases.py under IGN_RESIDENT=2: form 1 on the row-tile, in-degree and
    batch-boundary edges the table was built for."""
    s = sc.SHAPES[name]
    desc, dims, mi, plan, graphs, _, prm = sc.case_inputs(name)
    exp = rc.expected(graphs, s.kind, force_pg=True)
    assert exp["form"] == 1
    monkeypatch.setenv("IGN_RESIDENT", "2")
    _assert_info(name, _probe(plan, prm, graphs), exp)
    info = _resident_vs_batched(monkeypatch, desc, dims, mi, graphs, mode="2", seed=sc.SEED, bias=sc.BIAS)
    assert info["form"] >= 1, info


@pytest.mark.parametrize("group", [2, 3])
@pytest.mark.parametrize("name", sorted(rc.GROUPED))
def test_shapes_in_a_grouped_workgroup(monkeypatch, name, group):
    """The batch entries under IGN_RES_GROUP=2 and 3: a graph boundary inside a tile of the group's union."""
    desc, dims, mi, plan, graphs, _, prm = rc.case_inputs(name)
    exp = rc.case_expected(name, group=group)
    monkeypatch.setenv("IGN_RES_GROUP", str(group))
    monkeypatch.setenv("IGN_RESIDENT", "1")
    probe = _probe(plan, prm, graphs)
    _assert_info(name, probe, exp)
    assert probe["graphs_per_workgroup"] == group
    _resident_vs_batched(monkeypatch, desc, dims, mi, graphs, seed=sc.SEED, bias=sc.BIAS)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, c in rc.CASES.items() if c.grads))
def test_gradients_at_the_edge(monkeypatch, name):
    """The training forward (the SAVE instantiations: path-global on either side of edges A and D, with and
    without the message rows in LDS on either side of B) and the backward: _check_grads against float64
    autograd, then the same gradient bits from the per-MP training forward (IGN_RESIDENT_TRAIN=0)."""
    c = rc.case(name)
    _set_group(monkeypatch, c.group)
    desc, dims, _, _, graphs, labels, prm = rc.case_inputs(name)
    print(name, "train form", rc.case_expected(name)["train_form"])
    eng, b, grads = _check_grads(desc, dims, graphs, labels, prm, oracle=rc.grad_reference(name))
    base = grads.cpu().numpy()
    b.close()
    eng.close()
    assert np.abs(base).sum() > 0
    monkeypatch.setenv("IGN_RESIDENT_TRAIN", "0")
    eng, b, _, _, _, g = _engine_grads(desc, dims, graphs, labels, prm)
    got = g.cpu().numpy()
    b.close()
    eng.close()
    np.testing.assert_array_equal(got, base, err_msg="IGN_RESIDENT_TRAIN=0")
