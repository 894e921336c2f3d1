"""The table of tests/readout_op_cases.py on the GPU: the readout operations that run before predict
(pool_partial / pool_final / pool_ties / pool_bwd, product and product_bwd, gather and the extend CSR's
csr_gather_cols_add, concat_cols / split_cols_add around the neural_network ops) on their kernels' edges:
pooled widths 1 .. 300, 1 .. 8193 rows per graph around the 4096-row chunk, batches of 1 .. 64 graphs,
n-fold max ties with a gradient, every product broadcast, rows x F past the 16384-block grid cap.

Every bound is an existing one: test_gpu_parity's _close (TOL max(1, |y|) against the float64 DenseOracle) for
the inference forward's predictions, test_gpu_training's _check_grads (training forward, loss and l2 at 1e-5,
GTOL per gradient tensor) against float64 autograd.  In the observable entries predict is the identity, so
these bounds apply to the pooled / multiplied / gathered tensors themselves.  Everything else is bitwise."""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch

from ignnition_amd import _lib, partition, workloads
from ignnition_amd.engine import Batch, BatchedGraphs, Engine, MPPlan, device_count
from ignnition_amd.json_operations import Model_information
from tests import readout_op_cases as rc
from tests.readout_cases import _POOL
from tests.test_gpu_parity import TOL, _close, _scaled_err
from tests.test_gpu_training import GTOL, _check_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _engine(name, json_plan=False):
    desc, dims, _, plan, _, _, prm = rc.case_inputs(name)
    eng = Engine(plan, 0)
    if json_plan:
        h = C.c_void_p()
        _lib.check(_lib.lib.ign_plan_create_json(json.dumps(desc).encode(), json.dumps(dims).encode(), 0, C.byref(h)))
        _lib.lib.ign_plan_destroy(eng.handle)
        eng.handle = h
    eng.set_params(prm)
    return eng


def _narrowed(graphs):
    bg = BatchedGraphs.from_dicts(graphs)
    return BatchedGraphs({k: (v.astype(np.int32) if v.dtype == np.int64 else v, lens)
                          for k, (v, lens) in bg.arrays.items()}, bg.num_graphs)


def _step(eng, b, y):
    """One training forward, loss and backward on a batch: (predictions, loss, flat gradient)."""
    pred = b.forward_train().reshape(-1).copy()
    dpred = torch.empty_like(y)
    loss = eng.mse_loss(b.predictions_ptr(), y, dpred)
    grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    b.backward(dpred, grads)
    torch.cuda.synchronize()
    return pred, loss, grads.cpu().numpy()


def _run(name, graphs=None, labels=None, json_plan=False, narrow=False, train=True, twice=False):
    """A fresh engine under the current environment: the inference forward (and its replays from the captured
    hipGraph), then one training step, or two on the same batch."""
    g, l = rc.case_inputs(name)[4:6]
    graphs, labels = graphs or g, labels or l
    eng = _engine(name, json_plan)
    b = Batch(eng, _narrowed(graphs) if narrow else graphs)
    try:
        r = {"out": b.forward().reshape(-1).copy()}
        r["replay"] = [b.forward().reshape(-1).copy() for _ in range(2)]
        if train:
            b.enable_training()
            y = torch.tensor(np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in labels]), device="cuda")
            r["pred"], r["loss"], r["grads"] = _step(eng, b, y)
            if twice:
                r["again"] = _step(eng, b, y)
            r["named"] = {n: r["grads"][off:off + int(np.prod(shape))].reshape(shape) for n, shape, off in eng.layout}
        return r
    finally:
        b.close()
        eng.close()


_BASE = {}


def _base(name):
    """The default environment's run, once per case, shared by the tests (read-only)."""
    if name not in _BASE:
        _BASE[name] = _run(name)
    return _BASE[name]


def _same_bits(got, exp, what, keys=("out", "pred", "grads")):
    for k in keys:
        np.testing.assert_array_equal(got[k], exp[k], err_msg="%s: %s" % (what, k))
    assert got["loss"] == exp["loss"], what


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.ALL)
def test_forward_matches_oracle(name):
    """The inference forward (direct, and replayed twice from the captured hipGraph) and the training forward
    against DenseOracle."""
    ref = rc.reference(name).reshape(-1)
    r = _base(name)
    print("%s: %d predictions, max scaled error vs float64 oracle %.3g (inference) %.3g (training)"
          % (name, ref.size, _scaled_err(r["out"], ref), _scaled_err(r["pred"], ref)))
    _close(r["out"], ref)
    _close(r["pred"], ref)
    for o in r["replay"]:
        np.testing.assert_array_equal(o, r["out"])


@pytest.mark.parametrize("name", rc.ALL)
def test_gradients(name):
    """Loss, l2 and every gradient tensor against float64 autograd.

    Measured on an MI355X: the worst tensor of each entry lies between 5e-8 and 2.2e-5 relative L2 (stride: 1.7e-6).
    With its 16400 paths routed over 5 links instead of 1025, the stride entry missed GTOL on the GRU tensors
    (path_update/recurrent_kernel 2.4e-4): every link summed 3280 path states, and plain float32 autograd of
    that entry was itself 3e-5 from float64 (tests/test_readout_op_cases.py holds it below GTOL / 10)."""
    desc, dims, _, _, graphs, labels, prm = rc.case_inputs(name)
    print(name)
    eng, b, grads = _check_grads(desc, dims, graphs, labels, prm, oracle=rc.grad_reference(name))
    g = grads.cpu().numpy()
    b.close()
    eng.close()
    assert np.isfinite(g).all() and np.abs(g).sum() > 0


@pytest.mark.parametrize("name", [n for n in rc.TIES if rc.CASES[n].zero_gru])
def test_tie_gradient_is_the_analytic_value(name):
    """Every row of the tie column equals its bias: the n rows share the column's gradient, so the bias
    receives it once (not n times) and the kernel's column receives it times the rows' mean state.  (GTOL, a
    relative L2 bound on a tensor, is applied here to single entries of one: no looser for them.)"""
    col = rc.counts(name)["ties"][1]
    db, dk = rc.analytic_tie_gradient(name)
    g = _base(name)["named"]
    assert g[rc.op_param(0, 0, "bias")][col] == pytest.approx(db, rel=GTOL)
    assert g[rc.op_param(0, 0, "kernel")][0, col] == pytest.approx(dk[0], rel=GTOL)
    assert np.all(g[rc.op_param(0, 0, "kernel")][1:, col] == 0)


@pytest.mark.parametrize("name", [n for n in rc.EXTEND if any(rows for _, rows in rc.counts(n)["no_edge"])])
def test_rows_without_an_edge_keep_a_zero_gradient(name):
    """A link that no path crosses is read by no edge of extend_adjacencies and sends no message: its row of
    the extend backward's CSR is empty and its gradient row stays 0, so predictions, loss and every gradient
    keep their bits when that link's feature changes."""
    desc, dims, _, _, graphs, labels, prm = rc.case_inputs(name)
    (_, _), (_, idle) = rc.counts(name)["no_edge"]
    moved, off = [], 0
    for g in graphs:
        cap = np.array(g["link_capacity"], np.float32)
        for r in idle:
            if off <= r < off + int(g["num_link"]):
                cap[r - off] += np.float32(0.5)
        moved.append(dict(g, link_capacity=cap))
        off += int(g["num_link"])
    got = _run(name, graphs=moved)
    _same_bits(got, _base(name), "idle link's feature changed")


# ---------------------------------------------------------------------------------------------
# bitwise
@pytest.mark.parametrize("name", [n for n in rc.BITWISE if len(rc.CASES[n].graphs) > 1])
def test_batch_equals_graph_alone_and_rotated(name):
    """Pooling reduces per graph in a fixed order and a graph operand broadcasts over its own graph's rows:
    each graph's predictions in the batch are bitwise those of the graph alone and of the batch rotated by one."""
    graphs, labels = rc.case_inputs(name)[4:6]
    base = _base(name)
    parts = [_run(name, [g], [l], train=False)["out"] for g, l in zip(graphs, labels)]
    np.testing.assert_array_equal(np.concatenate(parts), base["out"], err_msg="graph by graph")
    rot = _run(name, list(graphs[1:]) + [graphs[0]], list(labels[1:]) + [labels[0]], train=False)["out"]
    np.testing.assert_array_equal(rot, np.concatenate(parts[1:] + parts[:1]), err_msg="rotated batch")


@pytest.mark.parametrize("env", [{"IGN_POOL": "0"}, {"IGN_POOL": "1", "IGN_POOL_POISON": "1"}], ids=["uncached", "poisoned"])
@pytest.mark.parametrize("name", rc.POISONED)
def test_pool_blocks_do_not_change_the_bits(monkeypatch, name, env):
    """Every backward of a readout operation adds into a gradient buffer: uncached blocks, and cached blocks
    that start as NaN, give the default run's bits (every buffer is cleared before it is added to)."""
    base = _base(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _same_bits(_run(name), base, " ".join("%s=%s" % kv for kv in env.items()))


@pytest.mark.parametrize("name", rc.BITWISE)
def test_json_plan_and_int32_indices_give_the_same_bits(name):
    base = _base(name)
    _same_bits(_run(name, json_plan=True), base, "ign_plan_create_json")
    _same_bits(_run(name, narrow=True), base, "int32 indices")


@pytest.mark.parametrize("name", rc.BITWISE)
def test_second_step_on_the_same_batch_gives_the_same_bits(name):
    """forward_train + backward twice on one batch: the second step's gradient buffers were used by the first."""
    r = _run(name, twice=True)
    pred, loss, grads = r["again"]
    np.testing.assert_array_equal(pred, r["pred"])
    assert loss == r["loss"]
    np.testing.assert_array_equal(grads.view(np.uint32), r["grads"].view(np.uint32))
    _same_bits(r, _base(name), "a second engine")


# ---------------------------------------------------------------------------------------------
# what is refused today, from both front ends.  tests/cpp/plan_lower_check.cpp pins the lowering's messages
# (products of widths 32 x 16 and 1 x 32, across entity row spaces, swapped extend inputs) on the ABI structs;
# here: that ign_plan_create and ign_plan_create_json give one status and one text for a description
_PROD = rc._PROD
_GATE = {"type": "neural_network", "nn_name": "gate", "input": ["path"], "output_name": "w"}
REFUSED = {
    "widths_1_32": ([_GATE, _PROD("w", "path", "o")], ["o"], {"gate": [(1, "sigmoid")]}, -2, "product of widths 1 and 32"),
    "widths_16_32": ([_GATE, _PROD("w", "path", "o")], ["o"], {"gate": [(16, "sigmoid")]}, -1, "product of widths 16 and 32"),
    "row_spaces": ([_PROD("path", "link", "o")], ["o"], None, -2, "product of tensors on different row spaces"),
    "extend_swapped": ([rc._EXT("link", "path")], ["ep"], None, -1,
                       "extend_adjacencies inputs must live on the adjacency's source and destination entities"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_plans(case):
    from ignnition_amd import model_examples
    ops, pin, nets, code, text = REFUSED[case]
    desc = model_examples.routenet_readout(ops, pin, nets, iterations=2)
    dims = rc.sc.dims("routenet")
    seen = []
    with pytest.raises(_lib.EngineError) as ei:
        Engine(MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)), 0)
    seen.append((ei.value.code, str(ei.value)))
    with pytest.raises(_lib.EngineError) as ei:
        h = C.c_void_p()
        _lib.check(_lib.lib.ign_plan_create_json(json.dumps(desc).encode(), json.dumps(dims).encode(), 0, C.byref(h)))
    seen.append((ei.value.code, str(ei.value)))
    assert seen[0] == seen[1]
    assert seen[0][0] == code and text in seen[0][1], seen[0]


@pytest.mark.parametrize("json_plan", [False, True], ids=["plan_create", "plan_create_json"])
def test_extend_index_outside_its_entity_is_refused_at_batch_creation(json_plan):
    """The host checks every index before anything is launched.  The adjacency of an extend_adjacencies is one
    that a message passing reads, and the batch lowers the message passings first: their check of the same
    index answers ("dst index ... out of range"); extend's own ("indexes outside its entities") stands behind it."""
    graphs = rc.case_inputs("ext_len1")[4]
    x = dict(graphs[0])
    x["dst_adj_paths_links"] = list(x["dst_adj_paths_links"])
    x["dst_adj_paths_links"][-1] = int(x["num_link"])
    eng = _engine("ext_len1", json_plan)
    try:
        with pytest.raises(_lib.EngineError, match="dst index 7 out of range") as ei:
            Batch(eng, [x])
        assert ei.value.code == -1
    finally:
        eng.close()


def test_readout_operations_on_an_edge_cut_partition_are_unsupported():
    desc, dims, mi, graphs, _ = workloads.make_synthetic_inputs(n_nodes=300, iterations=2, window=16)
    pred = desc["readout"][0]
    pred["input"] = ["g"]
    desc["readout"] = [_POOL("sum", "node", "g"), pred]
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    eng = Engine(plan, 0)
    eng.set_params(plan.init_params(1, bias_scale=0.1))
    p = partition.local_part(graphs[0], plan, 0, 2)
    assert sum(p.halos[n].n_halo for n in plan.entities) > 0
    try:
        with pytest.raises(_lib.EngineError, match="readout operations on an edge-cut partition") as ei:
            Batch(eng, [p.inputs], halo_rows={n: p.halos[n].n_halo for n in plan.entities})
        assert ei.value.code == -2
    finally:
        eng.close()
