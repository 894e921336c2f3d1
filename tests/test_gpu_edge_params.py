"""Per-edge parameters written into a live batch (Batch.set_edge_params) and the gradient of the loss
with respect to them (Batch.edge_param_gradients), on the GPU.

Gradients: against torch autograd of the float64 restatement with the params_<adj> arrays as leaves
(tests/edge_param_grad_oracle.py, pinned to the unchanged oracle by tests/test_edge_param_grad_oracle.py),
on the models of tests/edge_param_cases.py.  Labels and loss as tests/test_gpu_training.py's
_engine_grads makes them, and that file's bound, since these are the same backward kernels plus an
exact column add: per params_<adj> tensor
    ||g_engine - g_oracle|| <= 1e-4 ||g_oracle|| + 1e-7,
with every parameter gradient of the same step held to _check_grads' rule in the same run.

set_edge_params: bitwise against a fresh batch built with the new values, on every forward a
message-network plan can take (the graph-resident forward takes none: resident_plan_shape).

No case holds a graph without edges of the adjacency: ign_batch_create refuses such a graph ("adjacency
slot ... has no edges", the reference's scatter_nd shape max(seq) + 1 is undefined, GM:484-490)."""
import copy

import numpy as np
import pytest
import torch

from ignnition_amd._lib import EngineError
from ignnition_amd.engine import Batch, Engine, MPPlan, SplitBatch, device_count, edge_param_sources
from ignnition_amd.generate_model import ComnetModel
from ignnition_amd.json_operations import Model_information
from tests import edge_param_cases as ec
from tests.edge_param_grad_oracle import EdgeParamGradOracle

pytestmark = pytest.mark.gpu

GTOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


# ---------------------------------------------------------------------------------------------
def _plan(desc, dims):
    return MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))


def _engine(desc, dims, prm):
    eng = Engine(_plan(desc, dims), 0)
    eng.set_params(prm)
    return eng


def _labels_dev(labels):
    return torch.tensor(np.concatenate([np.asarray(l, np.float32).reshape(-1) for l in labels]), device="cuda")


def _train_step(eng, b, y):
    """forward_train, MSE loss, backward (as _engine_grads): predictions, loss, the flat parameter gradient."""
    pred = b.forward_train()
    dpred = torch.empty_like(y)
    loss = eng.mse_loss(b.predictions_ptr(), y, dpred)
    grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.backward(dpred, grads)
    torch.cuda.synchronize()
    return pred.copy(), loss, grads.cpu().numpy()


def _source_grads(eng, b, adj):
    """[the [edges, P] buffer of every (mp, source) that reads the adjacency's parameters]"""
    ne, P, sources = b._edge_sources(adj)
    out = []
    for m, k in sources:
        t = torch.full((ne, P), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        b.edge_param_source_gradients(m, k, t)
        eng.synchronize()
        out.append(t.cpu().numpy())
    return out


def _fresh_step(eng, graphs, y, adj):
    b = Batch(eng, graphs)
    b.enable_training(edge_param_gradients=True)
    out = _train_step(eng, b, y) + (b.edge_param_gradients(adj),)
    b.close()
    return out


# ---------------------------------------------------------------------------------------------
# gradients
@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_gradients(name):
    desc, dims, graphs, labels, prm = ec.case_inputs(name)
    adj = ec.ADJ[name]
    eng = _engine(desc, dims, prm)
    assert ec.slice_columns(eng.plan, adj) == ec.COLUMNS[name]
    b = Batch(eng, graphs)
    b.enable_training(edge_param_gradients=True)
    pred, loss, flat = _train_step(eng, b, _labels_dev(labels))
    g = b.edge_param_gradients(adj)
    per_source = _source_grads(eng, b, adj)
    ne, P, sources = b._edge_sources(adj)
    b.close()
    assert ne % 256 != 0 and g.shape == (ne, P) and g.dtype == np.float32
    o = EdgeParamGradOracle(desc, dims, prm)
    o_loss, _, o_g, o_pred = o.loss_and_grads(graphs, labels)
    o_eg = o.edge_param_grads()["params_" + adj]
    np.testing.assert_allclose(pred.reshape(-1), o_pred, rtol=1e-4, atol=1e-4)
    assert loss == pytest.approx(o_loss, rel=1e-5)
    named = {}
    for pname, shape, off in eng.layout:   # (two networks of one name: the oracle holds their sum)
        named[pname] = named.get(pname, 0) + flat[off:off + int(np.prod(shape))].reshape(shape).astype(np.float64)
    for pname, og in o_g.items():   # _check_grads' rule
        err = np.linalg.norm(named[pname] - og)
        assert err <= GTOL * np.linalg.norm(og) + 1e-7, "%s: rel err %.3g" % (pname, err / max(np.linalg.norm(og), 1e-30))
    err, n = np.linalg.norm(g.astype(np.float64) - o_eg), np.linalg.norm(o_eg)
    print("params_%s gradient vs float64 autograd: relative L2 %.3g (|g| %.3g)" % (adj, err / n, n))
    assert n > 0 and err <= GTOL * n + 1e-7, "rel err %.3g" % (err / n)
    # the per-source buffers, and the Python sum over them in plan order
    assert len(per_source) == len(sources) == (2 if name == "two_mps_p2" else 1)
    total = per_source[0].copy()
    for part in per_source[1:]:
        total += part
        assert np.abs(part).sum() > 0 and not np.array_equal(part, per_source[0])
    np.testing.assert_array_equal(g, total)
    eng.close()


# ---------------------------------------------------------------------------------------------
# set_edge_params
def _finish(eng, b):
    """A backward, so that the training forward's step is over: its parameter and edge-parameter gradients."""
    y = torch.linspace(-1, 1, b.predictions * b.output_units, dtype=torch.float32, device="cuda")
    dpred = torch.empty_like(y)
    eng.mse_loss(b.predictions_ptr(), y, dpred)
    g = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.backward(dpred, g)
    torch.cuda.synchronize()
    return g.cpu().numpy()


def _forward_stepped_inference(eng, b, adj):
    b.begin()
    for _ in range(eng.plan.iterations):
        for mi in range(len(eng.plan.mps)):
            b.run_mp(mi, "all")
    return (b.end().copy(),)


def _forward_train(eng, b, adj):
    out = b.forward_train().copy()
    return out, _finish(eng, b), b.edge_param_gradients(adj)


def _forward_train_stepped(eng, b, adj):
    b.forward_train_begin()
    for _ in range(eng.plan.iterations * len(eng.plan.mps)):
        b.forward_train_mp()
    out = b.forward_train_end().copy()
    return out, _finish(eng, b), b.edge_param_gradients(adj)


FORMS = {
    "captured_graph": ((), lambda eng, b, adj: (b.forward().copy(),)),
    "no_hip_graph": ((("IGN_HIP_GRAPH", "0"),), lambda eng, b, adj: (b.forward().copy(),)),
    "per_mp": ((), _forward_stepped_inference),
    "forward_train": ((), _forward_train),
    "forward_train_stepped": ((), _forward_train_stepped),
}


def _same(got, ref):
    assert len(got) == len(ref)
    for a, r in zip(got, ref):
        np.testing.assert_array_equal(a, r)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["sum_p3_last", "ordered_mixed", "attention_p2_last"])
def test_set_edge_params_is_bitwise(monkeypatch, name, form):
    """Parameters A, forward (twice: the second replays the captured graph), set B, forward: the
    predictions of a fresh batch built with B, and after a training forward its backward's parameter
    and edge-parameter gradients too; set A back: the first results."""
    env, run = FORMS[form]
    for k, v in env:
        monkeypatch.setenv(k, v)
    desc, dims, A, _, prm = ec.case_inputs(name)
    adj = ec.ADJ[name]
    B = ec.other_values(A, adj, 21)
    eng = _engine(desc, dims, prm)
    train = form.startswith("forward_train")

    def fresh(graphs):
        b = Batch(eng, graphs)
        if train:
            b.enable_training(edge_param_gradients=True)
        out = run(eng, b, adj)
        b.close()
        return out

    ref_a, ref_b = fresh(A), fresh(B)
    assert all(not np.array_equal(a, r) for a, r in zip(ref_a, ref_b))
    b = Batch(eng, A)
    if train:
        b.enable_training(edge_param_gradients=True)
    assert b.resident_info()["active"] == 0
    _same(run(eng, b, adj), ref_a)
    _same(run(eng, b, adj), ref_a)
    b.set_edge_params(adj, ec.edge_values(B, adj))
    _same(run(eng, b, adj), ref_b)
    _same(run(eng, b, adj), ref_b)
    b.set_edge_params(adj, ec.edge_values(A, adj).reshape(-1))   # flat
    _same(run(eng, b, adj), ref_a)
    b.close()
    eng.close()


def test_split_batch():
    """Edges sliced per sub-batch by their graphs' edge counts; the gradients of sub-batches that ran
    their own training steps, concatenated."""
    desc, dims, A, labels, prm = ec.case_inputs("sum_p2_middle")
    adj = ec.ADJ["sum_p2_middle"]
    B = ec.other_values(A, adj, 22)
    eng = _engine(desc, dims, prm)
    one = Batch(eng, B)
    ref_b = one.forward().copy()
    one.close()
    sb = SplitBatch(eng, A, parts=2)
    assert [int(p.graph_edges[:, 1].sum()) for p in sb.parts] == [406, 414]
    first = sb.forward().copy()
    sb.set_edge_params(adj, ec.edge_values(B, adj))
    np.testing.assert_array_equal(sb.forward(), ref_b)
    t = torch.from_numpy(ec.edge_values(A, adj)).cuda()
    torch.cuda.synchronize()
    sb.set_edge_params(adj, t)
    np.testing.assert_array_equal(sb.forward(), first)
    with pytest.raises(ValueError, match="the batch needs 820 rows of width 2"):
        sb.set_edge_params(adj, np.zeros((406, 2), np.float32))
    sb.set_edge_params(adj, ec.edge_values(B, adj))
    parts = []
    for k, p in enumerate(sb.parts):   # one graph each
        p.enable_training(edge_param_gradients=True)
        _train_step(p.engine, p, _labels_dev(labels[k:k + 1]))
        ref = _fresh_step(p.engine, B[k:k + 1], _labels_dev(labels[k:k + 1]), adj)
        parts.append(ref[3])
    g = sb.edge_param_gradients(adj)
    assert g.shape == (820, 2)
    np.testing.assert_array_equal(g, np.concatenate(parts))
    sb.close()
    eng.close()


def test_device_pointers_equal_the_host_path():
    """set_edge_params from a CUDA tensor and edge_param_gradients(out=tensor): the host path's bits."""
    name = "two_mps_p2"
    desc, dims, A, labels, prm = ec.case_inputs(name)
    adj = ec.ADJ[name]
    B = ec.other_values(A, adj, 5)
    eng = _engine(desc, dims, prm)
    y = _labels_dev(labels)
    ref = _fresh_step(eng, B, y, adj)
    dev = Batch(eng, A)
    dev.enable_training(edge_param_gradients=True)
    t = torch.from_numpy(ec.edge_values(B, adj)).cuda()
    torch.cuda.synchronize()
    dev.set_edge_params(adj, t)
    got = _train_step(eng, dev, y)
    _same(got, ref[:3])
    out = torch.full((820, 2), float("nan"), dtype=torch.float32, device="cuda")
    assert dev.edge_param_gradients(adj, out=out) is out
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), ref[3])
    with pytest.raises(ValueError, match="rows of width 2"):
        dev.edge_param_gradients(adj, out=torch.zeros((820, 1), device="cuda"))
    with pytest.raises(ValueError, match="rows of width 2"):
        dev.set_edge_params(adj, torch.zeros((819, 2), device="cuda"))
    dev.close()
    eng.close()


# ---------------------------------------------------------------------------------------------
# the opt-in
@pytest.mark.parametrize("name", ["sum_p4_middle", "ordered_p1_middle", "attention_p2_last"])
def test_opt_in_leaves_the_step_alone_and_is_reproducible(name):
    desc, dims, graphs, labels, prm = ec.case_inputs(name)
    adj = ec.ADJ[name]
    eng = _engine(desc, dims, prm)
    y = _labels_dev(labels)
    b = Batch(eng, graphs)
    b.enable_training()
    plain = _train_step(eng, b, y)
    with pytest.raises(EngineError, match="needs ign_batch_enable_edge_param_gradients"):
        b.edge_param_gradients(adj)
    _same(_train_step(eng, b, y), plain)
    b.enable_edge_param_gradients()
    with pytest.raises(EngineError, match="needs a completed backward of this batch that began after the opt-in"):
        b.edge_param_gradients(adj)   # the last backward kept nothing
    opted = _train_step(eng, b, y)
    g1 = b.edge_param_gradients(adj)
    _same(opted, plain)
    _same(_train_step(eng, b, y), plain)
    g2 = b.edge_param_gradients(adj)
    np.testing.assert_array_equal(g2, g1)
    assert np.abs(g1).sum() > 0 and np.all(np.isfinite(g1))
    b.close()
    fresh = _fresh_step(eng, graphs, y, adj)
    _same(fresh[:3], plain)
    np.testing.assert_array_equal(fresh[3], g1)
    eng.close()


# ---------------------------------------------------------------------------------------------
# refusals: each status and text as the ABI gives it, through the Python layer
def test_refusals():
    desc, dims, graphs, labels, prm = ec.case_inputs("sum_p3_last")
    adj = ec.ADJ["sum_p3_last"]
    A = ec.edge_values(graphs, adj)
    eng = _engine(desc, dims, prm)
    plan = eng.plan
    assert edge_param_sources(plan, adj) == (3, [(1, 0, 1)])
    b = Batch(eng, graphs)
    out = torch.zeros((820, 3), dtype=torch.float32, device="cuda")

    def refused(call, text, code=-1):
        with pytest.raises(EngineError, match=text) as e:
            call()
        assert e.value.code == code

    refused(lambda: b.edge_param_gradients(adj), "training not enabled")
    refused(b.enable_edge_param_gradients, "training not enabled")
    b.enable_training()
    refused(lambda: b.edge_param_gradients(adj), "needs ign_batch_enable_edge_param_gradients")
    b.enable_edge_param_gradients()
    refused(lambda: b.edge_param_gradients(adj), "needs a completed backward")   # no forward yet
    b.set_edge_params(adj, A)   # before any training forward: fine
    b.forward_train()
    refused(lambda: b.edge_param_gradients(adj), "needs a completed backward")   # the forward's backward has not run
    refused(lambda: b.set_edge_params(adj, A), "ign_batch_set_edge_params between a training forward and the end of its backward")
    y = _labels_dev(labels)
    dpred = torch.empty_like(y)
    eng.mse_loss(b.predictions_ptr(), y, dpred)
    grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.backward_begin(dpred, grads)
    for k in range(plan.iterations * len(plan.mps)):
        refused(lambda: b.set_edge_params(adj, A), "between a training forward and the end of its backward")
        refused(lambda: b.edge_param_gradients(adj), "needs a completed backward")
        b.backward_mp()
    b.backward_end()
    g = b.edge_param_gradients(adj)
    b.set_edge_params(adj, A)   # the step is over
    np.testing.assert_array_equal(b.edge_param_gradients(adj), g)   # still that backward's
    # (mp, source) without a message network, or whose network reads no edge_params; out of range
    for call in (lambda m, k: b.edge_param_source_gradients(m, k, out),
                 lambda m, k: _set_source(eng, b, m, k, A)):
        refused(lambda: call(0, 0), "source 0 of mp 0 has no message network")
        refused(lambda: call(2, 0), "mp index 2 out of range")
        refused(lambda: call(-1, 0), "mp index -1 out of range")
        refused(lambda: call(1, 1), "mp 1 has no source 1")
    b.forward_train()
    refused(lambda: b.edge_param_gradients(adj), "needs a completed backward")   # the next step began
    # from Python: names, rows and widths
    with pytest.raises(ValueError, match="the batch needs 820 rows of width 3"):
        b.set_edge_params(adj, np.zeros((821, 3), np.float32))
    with pytest.raises(ValueError, match="rows of width 3"):
        b.set_edge_params(adj, np.zeros((820, 2), np.float32))
    with pytest.raises(ValueError, match="rows of width 3"):
        b.set_edge_params(adj, torch.zeros((820, 2), device="cuda"))
    with pytest.raises(ValueError, match="no message network reads the edge parameters of adjacency 'adj_links_paths'"):
        b.set_edge_params("adj_links_paths", np.zeros((820, 3), np.float32))
    with pytest.raises(ValueError, match="no message network reads"):
        b.edge_param_gradients("adj_links_paths")
    b.close()
    eng.close()


def _set_source(eng, b, m, k, values):
    import ctypes as C
    from ignnition_amd._lib import check, lib
    check(lib.ign_batch_set_edge_params(eng.handle, b.handle, m, k, values.ctypes.data_as(C.c_void_p)))


def test_a_network_that_reads_no_edge_params_is_refused():
    from ignnition_amd import model_examples, synthetic, workloads
    desc = model_examples.routenet_message_net(inputs=("hs_source", "hs_dest"), units=(32,), activation="tanh", iterations=2)
    _, dims, _ = workloads.model("routenet")
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, labels = workloads.graph_inputs(mi, [synthetic.routenet_sample("nsfnet", 0)])
    eng = _engine(desc, dims, MPPlan.from_model_info(mi).init_params(6, bias_scale=0.1))
    b = Batch(eng, graphs)
    b.enable_training(edge_param_gradients=True)   # nothing to allocate: fine
    _train_step(eng, b, _labels_dev(labels))
    out = torch.zeros((406, 1), dtype=torch.float32, device="cuda")
    for call in (lambda: b.edge_param_source_gradients(1, 0, out), lambda: _set_source(eng, b, 1, 0, np.zeros((406, 1), np.float32))):
        with pytest.raises(EngineError, match="the message network of source 0 of mp 1 does not read edge_params") as e:
            call()
        assert e.value.code == -1
    with pytest.raises(ValueError, match="no message network reads"):
        b.set_edge_params("adj_paths_links", np.zeros((406, 1), np.float32))
    b.close()
    eng.close()


# ---------------------------------------------------------------------------------------------
def test_sensitivities():
    """ComnetModel.sensitivities(edge_params=True) on one NSFNET graph: the default call's entries to
    the bit, and params_<adj> = the autograd gradient of pred.sum()."""
    desc, dims, graphs, _, prm = ec.case_inputs("attention_p2_last")
    graphs = graphs[:1]
    m = ComnetModel(Model_information(copy.deepcopy(desc), dims), params=prm)
    pred, sens = m.sensitivities(graphs)
    assert set(sens) == {"link", "path"}
    pred2, sens2 = m.sensitivities(graphs, edge_params=True)
    assert set(sens2) == {"link", "path", "params_adj_paths_links"}
    np.testing.assert_array_equal(pred2, pred)
    for ent in sens:
        for name in sens[ent]:
            np.testing.assert_array_equal(sens2[ent][name], sens[ent][name])
    o_pred, o_eg = EdgeParamGradOracle(desc, dims, prm).sum_grads(graphs)
    np.testing.assert_allclose(pred.reshape(-1), o_pred, rtol=1e-4, atol=1e-4)
    og, g = o_eg["params_adj_paths_links"], sens2["params_adj_paths_links"]
    err, n = np.linalg.norm(g.astype(np.float64) - og), np.linalg.norm(og)
    print("params_adj_paths_links: relative L2 %.3g (|g| %.3g)" % (err / n, n))
    assert g.shape == (406, 2) and n > 0 and err <= GTOL * n + 1e-7
    m.engine.close()
