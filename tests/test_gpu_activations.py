"""elu, softplus, softsign, exponential and hard_sigmoid on the GPU (tests/activation_cases.py) against the
float64 oracles with the restatements patched in (the new_activations fixture).

Forward tolerance: test_gpu_parity's _ieee_tol rule with the IEEE float32 evaluation taken from the numpy
oracle at dtype float32 (the C++ restatement does not know these names): |engine - oracle| <=
max(1e-4, 1.5 x the float32 evaluation's own scaled error) x max(1, |oracle|), computed per case.
Gradients: test_gpu_training's rule (GTOL relative L2 per tensor)."""
import copy

import numpy as np
import pytest
import torch

from ignnition_amd.engine import Batch, Engine, MPPlan, device_count
from ignnition_amd.json_operations import Model_information
from oracle.dense_forward import DenseOracle
from oracle.train_oracle import TorchOracle, adam_step
from tests import activation_cases as ac
from tests import shape_cases as sc
from tests.activation_cases import new_activations   # noqa: F401 (the fixture)
from tests.test_gpu_parity import TOL, _scaled_err
from tests.test_gpu_training import GTOL, _check_grads, _engine_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")


def _tol(ieee, ref):
    yard = _scaled_err(ieee, ref)
    return yard, max(TOL, 1.5 * yard)


def _both_forwards(plan, prm, graphs):
    """(ign_forward's, the training forward's) predictions of a fresh engine on one batch."""
    eng = Engine(plan, 0)
    eng.set_params(prm)
    b = Batch(eng, graphs)
    out = np.array(b.forward()).reshape(-1)
    b.enable_training()
    train = np.array(b.forward_train()).reshape(-1)
    b.close()
    eng.close()
    return out, train


def _check_forward(what, plan, prm, graphs, ref, ieee):
    yard, tol = _tol(ieee, ref)
    for kind, got in zip(("inference", "training"), _both_forwards(plan, prm, graphs)):
        assert np.all(np.isfinite(got)), (what, kind)
        err = _scaled_err(got, ref)
        print("%s %s: max scaled error %.3g (float32 yardstick %.3g, tolerance %.3g)" % (what, kind, err, yard, tol))
        assert err <= tol, (what, kind, err, tol)


FORWARD = [(p, n) for p in ac.FORWARD_POSITIONS for n in ac.NAMES_AT[ac.FORWARD_AT[p]]]


@pytest.mark.parametrize("position,name", FORWARD)
def test_forward_positions(new_activations, position, name):
    """One name in one position on graphs of 1, 15, 16, 17 and 129 path rows (one batch each), the inference
    and the training forward: a predict hidden layer 32 and 16 wide, predict's last layer (act3), a readout
    neural_network operation, a message network's first layer (16 wide, per-edge rows) and its last (32 wide:
    the message the GRU reads) and the convolution's activation_function.  The layer's pre-activations cover
    the regimes of activation_cases.REGIMES."""
    desc, dims, plan, graphs, prm, ref, ieee = ac.forward_case(position, name, new_activations)
    assert np.ptp(np.concatenate(ref)) > 1e-3
    for p, g, r, i in zip(ac.ROWS, graphs, ref, ieee):
        _check_forward("%s %s P %d" % (position, name, p), plan, prm, [g], r, i)


@pytest.mark.parametrize("name", ac.NAMES_AT["message"])
def test_message_network_with_the_resident_switch(monkeypatch, new_activations, name):
    """A model with a message network is not resident-eligible: with the resident forward on (default) and off
    it runs the batched launches, the same bits."""
    desc, dims, plan, graphs, prm, ref, ieee = ac.forward_case("message", name, new_activations, rows=(17,))
    outs = {}
    for v in ("1", "0"):
        monkeypatch.setenv("IGN_RESIDENT", v)
        fresh = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
        eng = Engine(fresh, 0)
        eng.set_params(prm)
        eng.set_timing(True)
        outs[v] = np.array(Batch(eng, graphs).forward()).reshape(-1)
        assert eng.stats()["mp_resident"]["launches"] == 0
        eng.close()
    np.testing.assert_array_equal(outs["1"], outs["0"])
    assert _scaled_err(outs["1"], ref[0]) <= _tol(ieee[0], ref[0])[1]


def _grad_inputs(desc, rows=(17, 129), prefix=None, factor=1.0, shift=0.0):
    desc, dims = ac.no_normalization(desc), sc.dims("routenet")
    graphs = [sc.graph(sc.P_GRAPH[p]) for p in rows]
    _, _, labels, prm = sc.inputs_for(desc, dims, graphs)
    if prefix:
        prm = ac.scale_layer(prm, prefix, factor, shift)
    return desc, dims, graphs, labels, prm


# the factor on the hidden / message layer: elu's both arms, hard_sigmoid rows exactly at 0 and at 1 (its
# pre-activations reach beyond +-2.5), softplus' and exponential's growth
GRAD_FACTOR = {"elu": 4.0, "softplus": 16.0, "softsign": 8.0, "exponential": 6.0, "hard_sigmoid": 16.0}


@pytest.mark.parametrize("name", ac.NAMES)
def test_gradients_predict_and_message_network(new_activations, name):
    """A 32 -> 16 ``name`` -> 1 predict stack behind a two-layer message network (16 ``name``, 32 tanh;
    softsign where ``name`` is refused in a message layer): ign_backward against torch autograd of the float64
    restatement on the same parameters."""
    desc = ac.message_model(name if name in ac.NAMES_AT["message"] else "softsign")
    ac._readout_net(desc)[:] = [{"type_layer": "Dense", "name": "hid", "units": 16, "activation": name},
                                {"type_layer": "Dense", "name": "out", "units": 1, "activation": "None"}]
    desc, dims, graphs, labels, prm = _grad_inputs(desc)
    prm = ac.scale_layer(prm, "readout_model_0/hid/", GRAD_FACTOR[name])
    prm = ac.scale_layer(prm, "path_to_link_message_creation_0/layer_0", GRAD_FACTOR[name])
    del new_activations[:]
    DenseOracle(desc, dims, prm).forward(graphs)
    z = np.concatenate(new_activations)
    assert (z < 0).mean() >= 0.1 and (z > 0).mean() >= 0.1
    if name == "hard_sigmoid":   # outputs exactly 0 and exactly 1: zero gradient in both
        a = ac.act_np(z, name)
        assert (a == 0).mean() >= 0.05 and (a == 1).mean() >= 0.05
    _check_grads(desc, dims, graphs, labels, prm)


@pytest.mark.parametrize("name", ac.CONV_NAMES)
def test_gradients_convolution(new_activations, name):
    desc, dims, graphs, labels, prm = _grad_inputs(ac.conv_model(name), prefix="convolution/", factor=8.0)
    _check_grads(desc, dims, graphs, labels, prm)


@pytest.mark.parametrize("second", ["softplus", "selu"])
def test_gradients_wide_layers(new_activations, second):
    """256 elu, 256 softplus, 1: the K = 256 split-fp16 Dense kernel with a new activation (layer 2's
    forward) and its transposed backward followed by the derivative's own launch.  256 elu, 256 selu, 1:
    that launch behind a layer whose own rows the output layer's fused backward formed."""
    desc = ac.predict_model("elu", 0, acts=("selu", second, "None"))
    _check_grads(*_grad_inputs(desc))


@pytest.mark.parametrize("name", [n for n in ac.NAMES if n != "exponential"])
def test_gradients_k64_k128(new_activations, name):
    """H = 64 states into 128 ``name``, 128 ``name``, 1: dense_h16's K = 64 and K = 128 instantiations of the
    new activations in the training forward, their derivatives behind dense_h16_t.  (A plan that names
    exponential stays off these kernels: test_exponential_far_beyond_fp16_range.)"""
    desc = ac.predict_model(name, 0, hidden=64, widths=(128, 128, 1), acts=("selu", name, "None"))
    _check_grads(*_grad_inputs(desc, rows=(17,)))


def test_softplus_deep_negative_gradients(new_activations):
    """Every hidden pre-activation of a 32 -> 16 softplus -> 1 stack below -15 (bias -17): a = exp(z) lies
    under float32's 1 + a == 1, so log(1 + exp(z)) or 1 - exp(-a) taken literally are 0.  The hidden
    layer's gradients within GTOL of the oracle's relative to their own (tiny) norm, no absolute slack."""
    desc = ac.predict_model("softplus", 0, widths=(16, 1), acts=("selu", "None"))
    desc, dims, graphs, labels, prm = _grad_inputs(desc, rows=(17,))
    prm["readout_model_0/predict_0/bias"] = np.full_like(prm["readout_model_0/predict_0/bias"], -17.0)
    del new_activations[:]
    DenseOracle(desc, dims, prm).forward(graphs)
    assert np.concatenate(new_activations).max() < -15
    eng, b, pred, loss, g, _ = _engine_grads(desc, dims, graphs, labels, prm)
    _, _, o_g, o_pred = TorchOracle(desc, dims, prm).loss_and_grads(graphs, labels)
    np.testing.assert_allclose(pred.reshape(-1), o_pred, rtol=1e-4, atol=1e-4)
    for k in ("readout_model_0/predict_0/kernel", "readout_model_0/predict_0/bias", "readout_model_0/predict_1/kernel"):
        ref = np.linalg.norm(o_g[k])
        assert 0 < ref < 1e-4, (k, ref)
        err = np.linalg.norm(g[k].astype(np.float64) - o_g[k])
        print("%s: |g| %.3g, relative error %.3g" % (k, ref, err / ref))
        assert err <= GTOL * ref, (k, err / ref)


def test_exponential_ahead_of_a_scaled_layer(new_activations):
    """256 exponential, 256 selu, 1 at 17 rows, layer 1's pre-activations reaching about +-10: layer 2's
    input reaches e^10, far beyond the bound 1.0508 |z| + 1.7582 the fused readouts' fp16 scales assume.
    Finite and within the per-case float32 yardstick, in inference (fp32 operands) and in the training
    forward (split-bf16 pieces, no scale)."""
    desc = ac.no_normalization(ac.predict_model("exponential", 0))
    dims, graphs = sc.dims("routenet"), [sc.graph(sc.P_GRAPH[17])]
    _, plan, _, prm = sc.inputs_for(desc, dims, graphs)
    del new_activations[:]
    DenseOracle(desc, dims, prm).forward(graphs)
    z0 = np.concatenate(new_activations)
    prm = ac.scale_layer(prm, "readout_model_0/predict_0/", 10.0 / np.abs(z0 - z0.mean()).max(), z0.mean())
    del new_activations[:]
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    z = np.concatenate(new_activations)
    assert 9.0 <= z.max() <= 11.0 and -11.0 <= z.min() <= -5.0, (z.min(), z.max())
    ieee = DenseOracle(desc, dims, prm, dtype=np.float32).forward(graphs)
    assert np.all(np.isfinite(ieee))
    _check_forward("exponential 256-256-1", plan, prm, graphs, ref, ieee)


def test_exponential_far_beyond_fp16_range(new_activations):
    """The same readout with layer 1's pre-activations reaching 80: exp(80) = 5.5e34 is finite in float32 and
    so is everything behind it (asserted on the float32 numpy evaluation), but it lies 2^40 above what a
    tile scale of the split-fp16 Dense kernel can bring into fp16 range (exponent clamp at 2^-60).  Both
    forwards finite and within the float32 yardstick: such a plan runs on exact split-bf16 pieces and fp32."""
    desc = ac.no_normalization(ac.predict_model("exponential", 0))
    dims, graphs = sc.dims("routenet"), [sc.graph(sc.P_GRAPH[17])]
    _, plan, _, prm = sc.inputs_for(desc, dims, graphs)
    del new_activations[:]
    DenseOracle(desc, dims, prm).forward(graphs)
    z0 = np.concatenate(new_activations)
    prm = ac.scale_layer(prm, "readout_model_0/predict_0/", 80.0 / np.abs(z0 - z0.mean()).max(), z0.mean())
    del new_activations[:]
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    z = np.concatenate(new_activations)
    assert 75.0 <= z.max() <= 81.0, z.max()
    assert np.exp(np.float32(z.max())) < np.float32(np.inf) and np.exp(z.max()) > 2.0 ** 75 * 2.0 ** 15
    with np.errstate(over="raise"):
        ieee = DenseOracle(desc, dims, prm, dtype=np.float32).forward(graphs)
    assert np.all(np.isfinite(ieee)) and np.abs(ref).max() > 1e30
    _check_forward("exponential to z = 80", plan, prm, graphs, ref, ieee)


@pytest.mark.parametrize("layer", [0, 1, 2])
@pytest.mark.parametrize("name", ac.NAMES)
def test_no_silent_linear(monkeypatch, new_activations, name, layer):
    """The 256-selu-256-selu-1 net of the fused readouts with one layer's activation replaced, under every
    readout variant: the plan leaves the fused kernels (or they gained the case), never the identity."""
    desc = ac.no_normalization(ac.predict_model(name, layer))
    dims, graphs = sc.dims("routenet"), [sc.graph(sc.P_GRAPH[17])]
    _, _, _, prm = sc.inputs_for(desc, dims, graphs)
    ref = DenseOracle(desc, dims, prm).forward(graphs)
    linear = DenseOracle(ac.no_normalization(ac.predict_model("None", layer)), dims, prm).forward(graphs)
    ieee = DenseOracle(desc, dims, prm, dtype=np.float32).forward(graphs)
    tol = _tol(ieee, ref)[1]
    assert _scaled_err(linear, ref) > 10 * tol   # the identity in its place would not pass
    for v in ("1", "2", "4", "5"):
        monkeypatch.setenv("IGN_READOUT_VARIANT", v)
        plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
        _check_forward("%s layer %d variant %s" % (name, layer, v), plan, prm, graphs, ref, ieee)


def test_one_adam_step_elu_readout_softplus_messages(new_activations):
    """elu in the readout, softplus in a message network: the gradients against autograd, then one Adam step
    against the float64 Keras restatement (test_adam_step_matches_keras_restatement's bounds), and the
    repacked fragments: a forward after the step equals a fresh engine's on the same parameters."""
    desc = ac.message_model("softplus")
    for l in ac._readout_net(desc)[:2]:
        l["activation"] = "elu"
    desc, dims, graphs, labels, prm = _grad_inputs(desc, rows=(17, 129))
    eng, b, grads = _check_grads(desc, dims, graphs, labels, prm)
    g = grads.cpu().numpy()
    named = {n: g[off:off + int(np.prod(shape))].reshape(shape) for n, shape, off in eng.layout}
    m, v = torch.zeros_like(grads), torch.zeros_like(grads)
    ref = {k: np.asarray(x, np.float64) for k, x in prm.items()}
    rm = {k: np.zeros_like(x) for k, x in ref.items()}
    rv = {k: np.zeros_like(x) for k, x in ref.items()}
    eng.adam_step(grads, m, v, 0, 0.01)
    adam_step(ref, {k: named[k].astype(np.float64) for k in ref}, rm, rv, 0, 0.01)
    got = eng.get_params()
    for k in ref:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-5, atol=1e-6, err_msg=k)
    fresh = Engine(MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims)), 0)
    fresh.set_params(got)
    np.testing.assert_array_equal(Batch(fresh, graphs).forward(), Batch(eng, graphs).forward())
