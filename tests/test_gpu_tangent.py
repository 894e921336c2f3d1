"""Batch.forward_tangent (ign_forward_tangent, tangent.hip): J.v of the predictions along one direction of
the input features, against float64 autograd of the restated model with the feature columns as leaves
(tests/input_grad_oracle.py; J.v row by row: one reverse pass per prediction and a product with v).

Every case: T = 2, init_params(5, bias_scale=0.1), graphs from tests/shape_cases.py's builders, v standard
normal over every feature of every entity (seed 3).  Bounds, the project's own:
dpred within 1e-4 relative L2 of J.v over the batch, pred within 1e-4 max(1, |ref|), and the adjoint
identity |<d, dpred> - <g, v>| <= 1e-4 (|d| |J.v| + |g| |v|) against feature_gradients after backward(d).
The Dropout case's reverse side runs on the same model without the Dropout layer: a training forward draws
a mask, so it is another function than the inference forward whose tangent this is."""
import copy
import functools

import numpy as np
import pytest
import torch

from ignnition_amd._lib import EngineError
from ignnition_amd.engine import Batch, Engine, MPPlan, device_count
from ignnition_amd.generate_model import ComnetModel
from ignnition_amd.json_operations import Model_information
from tests import activation_cases, aggregation_cases, edge_param_cases
from tests import shape_cases as sc
from tests.activation_cases import new_activations   # noqa: F401  (softplus in the torch oracle)
from tests.input_grad_oracle import CellInputGradOracle
from tests.shape_cases import G, _one_long, _rand

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _c(*graphs, kind="routenet", link=32, path=32, cell=None, predict=None):
    return dict(graphs=graphs, kind=kind, link=link, path=path, cell=cell or {}, predict=predict)


_P17 = G(17, 5, _rand(17, 4))
_OPTIONS = {"v1": {"reset_after": False}, "no_bias": {"use_bias": False},
            "softsign": {"activation": "softsign", "recurrent_activation": "sigmoid"}}
_SOFTPLUS = [{"type_layer": "Dense", "name": "predict_0", "units": 32, "activation": "selu"},
             {"type_layer": "Dropout", "rate": 0.25},
             {"type_layer": "Dense", "name": "predict_1", "units": 16, "activation": "softplus"},
             {"type_layer": "Dense", "name": "predict_2", "units": 1, "activation": "None"}]
CASES = {
    # the 16-row tile edge of both kernels: paths 1, 16, 17 over 2 and over 17 links
    "p1_l2": _c(G(1, 2, (2,))), "p16_l2": _c(G(16, 2, _rand(16, 2))), "p17_l2": _c(G(17, 2, _rand(17, 2))),
    "p1_l17": _c(G(1, 17, (17,))), "p16_l17": _c(G(16, 17, _rand(16, 4))), "p17_l17": _c(G(17, 17, _rand(17, 4))),
    # one long path among length-1 paths: masked lanes pass hd through
    "long17_first": _c(G(20, 17, _one_long(20, 17, 0))), "long17_last": _c(G(20, 17, _one_long(20, 17, 19))),
    "l16_idle": _c(G(40, 16, _rand(40, 3, 7), idle_links=1)),    # a destination without a message
    "deg65": _c(G(80, 4, _rand(80, 3, 12), hot=65)),             # link 0 takes the segmented sum
    "b17_1_15": _c(G(17, 17, _rand(17, 3, 16)), G(1, 1, 1, seed=1), G(15, 15, _rand(15, 3, 17), seed=2)),
    "h16": _c(_P17, link=16, path=16), "h64": _c(_P17, link=64, path=64),
    "l16_p32": _c(_P17, link=16, path=32), "l32_p16": _c(_P17, link=32, path=16),
    "qsize": _c(G(20, 6, _rand(20, 4, 22), N=17), kind="qsize"),  # two interleaved sources, two sum MPs
    "softplus_dropout": _c(_P17, predict=_SOFTPLUS),
}
CASES.update({"%s_h%d" % (n, h): _c(_P17, link=h, path=h, cell=o) for n, o in _OPTIONS.items() for h in (32, 64)})


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(desc, the same without Dropout layers, dims, plan, graphs, parameters)."""
    c = CASES[name]
    desc, dims = sc.model(c["kind"], 32)
    for e in desc["entities"]:
        e["hidden_state_dimension"] = c["link"] if e["name"] != "path" else c["path"]
    for n in desc["neural_networks"]:
        if n["nn_name"] == "recurrent1":
            n.update(c["cell"])
        if n["nn_name"] == "readout_model" and c["predict"]:
            n["nn_architecture"] = copy.deepcopy(c["predict"])
    plain = copy.deepcopy(desc)
    for n in plain["neural_networks"]:
        if "nn_architecture" in n:
            n["nn_architecture"] = [l for l in n["nn_architecture"] if l["type_layer"] != "Dropout"]
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    return desc, plain, dims, plan, [sc.graph(g, c["kind"]) for g in c["graphs"]], plan.init_params(sc.SEED, bias_scale=sc.BIAS)


def _direction(plan, graphs, seed=3):
    """{entity: {feature: [rows of the batch, size]}}, standard normal."""
    rng = np.random.default_rng(seed)
    return {ent: {f: rng.standard_normal((sum(int(g["num_" + ent]) for g in graphs), size)).astype(np.float32)
                  for f, size in feats} for ent, feats in zip(plan.entities, plan.features) if feats}


def _jvp64(plain, dims, plan, graphs, prm, v):
    """(predictions, J.v) of the float64 restatement, one reverse pass per prediction."""
    o = CellInputGradOracle(plain, dims, prm)
    pred = o.forward(graphs)
    leaves, parts = [], []
    for ent, feats in v.items():
        r0 = 0
        for gi, g in enumerate(graphs):
            n = int(g["num_" + ent])
            for f in feats:
                leaves.append(o.leaves[gi][f])
                parts.append(torch.tensor(feats[f][r0:r0 + n].astype(np.float64)))
            r0 += n
    jv = np.zeros(pred.numel())
    for i in range(pred.numel()):
        gs = torch.autograd.grad(pred[i], leaves, retain_graph=True, allow_unused=True)
        jv[i] = sum(float((g * p).sum()) for g, p in zip(gs, parts) if g is not None)
    return pred.detach().numpy(), jv


@functools.lru_cache(maxsize=None)
def _reference(name, seed=sc.SEED):
    desc, plain, dims, plan, graphs, prm = _inputs(name)
    if seed != sc.SEED:
        prm = plan.init_params(seed, bias_scale=sc.BIAS)
    return _jvp64(plain, dims, plan, graphs, prm, _direction(plan, graphs))


def _open(desc, dims, graphs, prm):
    eng = Engine(MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)), 0)
    eng.set_params(prm)
    return eng, Batch(eng, graphs)


def _rel(a, ref):
    return np.linalg.norm(a.astype(np.float64).reshape(-1) - ref) / np.linalg.norm(ref)


@pytest.mark.parametrize("name", sorted(CASES))
def test_tangent(name, new_activations):   # noqa: F811
    desc, plain, dims, plan, graphs, prm = _inputs(name)
    v = _direction(plan, graphs)
    ref, jv = _reference(name)
    assert np.linalg.norm(jv) > 0
    eng, b = _open(desc, dims, graphs, prm)
    pred, dpred = b.forward_tangent(v)
    b.close()
    eng.close()
    print("%s: dpred relative L2 %.3g, pred max scaled error %.3g"
          % (name, _rel(dpred, jv), (np.abs(pred.reshape(-1) - ref) / np.maximum(1, np.abs(ref))).max()))
    assert _rel(dpred, jv) <= TOL
    assert np.all(np.abs(pred.reshape(-1) - ref) <= TOL * np.maximum(1, np.abs(ref)))
    # the adjoint identity against the reverse mode
    eng, b = _open(plain, dims, graphs, prm)
    b.enable_training()
    b.forward_train()
    d = np.random.default_rng(9).standard_normal(dpred.size).astype(np.float32)
    grads = torch.zeros(eng.n_params, dtype=torch.float32, device="cuda")
    dd = torch.from_numpy(d).cuda()
    torch.cuda.synchronize()
    b.backward(dd, grads)
    g = {ent: b.feature_gradients(ent) for ent in v}
    b.close()
    eng.close()
    gv = sum(float((g[e][f].astype(np.float64) * v[e][f]).sum()) for e in v for f in v[e])
    ng = np.sqrt(sum(float((g[e][f].astype(np.float64) ** 2).sum()) for e in v for f in v[e]))
    nv = np.sqrt(sum(float((v[e][f].astype(np.float64) ** 2).sum()) for e in v for f in v[e]))
    lhs = float(d.astype(np.float64) @ dpred.astype(np.float64).reshape(-1))
    assert abs(lhs - gv) <= TOL * (np.linalg.norm(d) * np.linalg.norm(jv) + ng * nv)


def test_zero_direction_linearity_and_an_untouched_batch():
    desc, _, dims, plan, graphs, prm = _inputs("qsize")
    v = _direction(plan, graphs)
    eng, b = _open(desc, dims, graphs, prm)
    before, states = b.forward().copy(), {e: b.state(e) for e in plan.entities}
    pred, dpred = b.forward_tangent(v)
    pred0, dpred0 = b.forward_tangent({})
    _, dpred2 = b.forward_tangent({e: {f: 2 * a for f, a in fs.items()} for e, fs in v.items()})
    after = b.forward()
    assert np.all(dpred0 == 0) and np.array_equal(pred0, pred)      # the primal does not read the tangent
    assert np.any(dpred != 0) and np.array_equal(dpred2, 2 * dpred)  # a power of two commutes with every rounding
    assert np.array_equal(before, after)
    for e in plan.entities:
        assert np.array_equal(states[e], b.state(e))
    with pytest.raises(ValueError, match="no entity"):
        b.forward_tangent({"router": np.zeros(3)})
    with pytest.raises(ValueError, match="forward_tangent: .*shape"):
        b.forward_tangent({"link": np.zeros((b.rows[0] + 1, 1))})
    b.close()
    eng.close()


def test_parameters_are_live():
    """A default-cell model: the raw fragments are packed from the parameters of the call."""
    desc, _, dims, plan, graphs, prm = _inputs("p17_l17")
    eng, b = _open(desc, dims, graphs, prm)
    first = b.forward_tangent(_direction(plan, graphs))[1]
    eng.set_params(plan.init_params(6, bias_scale=sc.BIAS))
    second = b.forward_tangent(_direction(plan, graphs))[1]
    b.close()
    eng.close()
    assert _rel(first, _reference("p17_l17")[1]) <= TOL and _rel(second, _reference("p17_l17", 6)[1]) <= TOL
    assert _rel(second, _reference("p17_l17")[1]) > 100 * TOL
    # the model-level call: directions per feature name, a feature left out does not move
    model = ComnetModel(Model_information(copy.deepcopy(desc), dims), params=prm)
    v = _direction(plan, graphs)
    both = model.directional_sensitivities(graphs, {"traffic": v["path"]["traffic"], "link_capacity": v["link"]["link_capacity"]})
    assert np.array_equal(both[1], first)
    only = model.directional_sensitivities(graphs, {"traffic": v["path"]["traffic"]})
    assert np.array_equal(only[0], both[0]) and not np.array_equal(only[1], first)
    with pytest.raises(ValueError, match="unknown feature"):
        model.directional_sensitivities(graphs, {"delay": v["path"]["traffic"]})
    model.engine.close()


def _refusals():
    a = aggregation_cases.case_inputs("att_l1")
    yield "attention", a[0], a[1], a[4], a[6], False
    desc, dims, graphs, _, prm = edge_param_cases.case_inputs("sum_p1_first")
    yield "message network", desc, dims, graphs, prm, False
    desc = activation_cases.no_normalization(activation_cases.readout_op_model("tanh"))
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), sc.dims("routenet")))
    yield "readout operation", desc, sc.dims("routenet"), [sc.graph(_P17)], plan.init_params(sc.SEED, bias_scale=sc.BIAS), False
    desc, _, dims, _, graphs, prm = _inputs("p17_l2")
    yield "training step", desc, dims, graphs, prm, True


@pytest.mark.parametrize("what", ["attention", "message network", "readout operation", "training step"])
def test_refused_by_name(what):
    _, desc, dims, graphs, prm, train = next(r for r in _refusals() if r[0] == what)
    eng, b = _open(desc, dims, graphs, prm)
    if train:
        b.enable_training()
        b.forward_train()
    with pytest.raises(EngineError, match="forward tangent: .*" + what):
        b.forward_tangent({})
    b.close()
    eng.close()
