"""The elementwise Keras activations beyond linear / relu / selu / sigmoid / tanh (tf.keras.activations,
TF 2.x): elu (alpha 1), softplus, softsign, exponential, hard_sigmoid (clip(0.2 z + 0.5, 0, 1)).

The oracles (oracle/dense_forward.py, oracle/train_oracle.py) do not restate them, so this module does, in
numpy (dtype-preserving: float64 for the reference, float32 for the IEEE yardstick) and in torch (autograd),
from library functions and not from the engine's formulas (expm1, logaddexp, clip), and the
``new_activations`` fixture puts them in front of the two oracles' ``_act`` for one test.  grad_out is each
derivative as a function of the activation's OUTPUT, the form the engine's backward uses on the saved
activations; tests/test_activation_host.py checks both against finite differences.

The models put one of the names in each position an activation code travels through: a predict Dense
layer, a readout neural_network operation, a message-creation network and the convolution aggregation's
activation_function.  No GPU is needed here."""
import copy

import numpy as np
import pytest
import torch

from ignnition_amd import model_examples

CODES = {"elu": 5, "softplus": 6, "softsign": 7, "exponential": 8, "hard_sigmoid": 9}
NAMES = sorted(CODES, key=CODES.get)
# Position / name pairs that stay refused because existing tests pin them: softplus as a
# convolution activation_function (tests/test_plan.py); code 9 there and in a message layer, code 5 in a
# readout operation's Dense layer (tests/cpp/plan_lower_check.cpp)
REFUSED_AT = {"predict": [], "readout_op": ["elu"], "message": ["hard_sigmoid"], "convolution": ["softplus", "hard_sigmoid"]}
NAMES_AT = {pos: [n for n in NAMES if n not in ref] for pos, ref in REFUSED_AT.items()}
CONV_NAMES = NAMES_AT["convolution"]
REFUSED = ["swish", "softmax", "no_such_activation"]


def act_np(x, name):
    if name == "elu":
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    if name == "softplus":
        return np.logaddexp(0, x)
    if name == "softsign":
        return x / (1 + np.abs(x))
    if name == "exponential":
        return np.exp(x)
    if name == "hard_sigmoid":
        return np.clip(0.2 * x + 0.5, 0, 1)
    raise KeyError(name)


def act_torch(x, name):
    if name == "elu":
        return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0)))
    if name == "softplus":
        return torch.logaddexp(torch.zeros_like(x), x)
    if name == "softsign":
        return x / (1 + torch.abs(x))
    if name == "exponential":
        return torch.exp(x)
    if name == "hard_sigmoid":
        return torch.clamp(0.2 * x + 0.5, 0, 1)
    raise KeyError(name)


def grad_out(a, name):
    """act'(z) through a = act(z), float64."""
    a = np.asarray(a, np.float64)
    if name == "elu":
        return np.where(a > 0, 1.0, a + 1.0)
    if name == "softplus":
        return -np.expm1(-a)
    if name == "softsign":
        return (1 - np.abs(a)) ** 2
    if name == "exponential":
        return a
    if name == "hard_sigmoid":
        return np.where((a > 0) & (a < 1), 0.2, 0.0)
    raise KeyError(name)


@pytest.fixture
def new_activations(monkeypatch):
    """oracle.dense_forward._act and oracle.train_oracle._act know NAMES for the duration of the test.
    Returns the list the float64 numpy oracle's pre-activations of those names are appended to."""
    import oracle.dense_forward as dense
    import oracle.train_oracle as train
    np_act, torch_act = dense._act, train._act
    seen = []

    def numpy_act(x, name):
        if name not in CODES:
            return np_act(x, name)
        if np.asarray(x).dtype == np.float64:
            seen.append(np.array(x, np.float64).reshape(-1))
        return act_np(x, name)

    monkeypatch.setattr(dense, "_act", numpy_act)
    monkeypatch.setattr(train, "_act", lambda x, name: act_torch(x, name) if name in CODES else torch_act(x, name))
    return seen


# ---------------------------------------------------------------------------------------------
# the four positions
def _readout_net(desc):
    return [n for n in desc["neural_networks"] if n["nn_name"] == "readout_model"][0]["nn_architecture"]


def predict_model(name, layer=0, hidden=32, iterations=2, widths=(256, 256, 1), acts=("selu", "selu", "None")):
    """RouteNet whose predict stack has ``widths`` / ``acts``, layer ``layer``'s activation replaced by ``name``."""
    d = model_examples.routenet(hidden=hidden, iterations=iterations)
    arch = [{"type_layer": "Dense", "name": "predict_%d" % i, "units": u, "activation": a}
            for i, (u, a) in enumerate(zip(widths, acts))]
    arch[layer]["activation"] = name
    for n in d["neural_networks"]:
        if n["nn_name"] == "readout_model":
            n["nn_architecture"] = arch
    return d


def readout_op_model(name, units=16, hidden=32, iterations=2):
    """A one-layer neural_network operation on the path states in front of a linear 1-unit predict."""
    op = {"type": "neural_network", "nn_name": "emb", "input": ["path"], "output_name": "pe"}
    d = model_examples.routenet_readout([op], ["pe"], {"emb": [(units, name)]}, hidden=hidden, iterations=iterations)
    _readout_net(d)[:] = [{"type_layer": "Dense", "name": "out", "units": 1, "activation": "None"}]
    return d


def message_model(name, units=(16, 32), hidden=32, iterations=2):
    """path -> link messages from a message-creation network on (hs_source, hs_dest): ``name`` on its first
    layer, tanh on its last (the messages a GRU reads stay bounded whatever ``name`` grows to)."""
    d = model_examples.routenet_message_net(inputs=("hs_source", "hs_dest"), units=units, activation=name,
                                            hidden=hidden, iterations=iterations)
    [n for n in d["neural_networks"] if n["nn_name"] == "message_nn"][0]["nn_architecture"][-1]["activation"] = "tanh"
    return d


def message_last_model(name, units=(16, 32), hidden=32, iterations=2):
    """The same network with tanh on its first layer and ``name`` on its 32-wide last one: the message the
    GRU reads is ``name``'s output."""
    d = message_model("tanh", units, hidden, iterations)
    [n for n in d["neural_networks"] if n["nn_name"] == "message_nn"][0]["nn_architecture"][-1]["activation"] = name
    return d


def conv_model(name, hidden=32, iterations=2):
    return model_examples.routenet_aggregation({"type": "convolution", "activation_function": name}, hidden=hidden,
                                               iterations=iterations)


POSITIONS = {"predict": predict_model, "readout_op": readout_op_model, "message": message_model, "convolution": conv_model}


def plan_activations(plan):
    """The activation codes of an MPPlan in the layout of ign_plan_describe_json's "activations"."""
    return {"predict": [l[2] for l in plan.dense],
            "readout_ops": [[l[2] for l in op["layers"]] for op in plan.readout_ops],
            "message": [[[l[2] for l in net["layers"]] if net else [] for net in mp["nets"]] for mp in plan.mps],
            "convolution": [int(mp.get("act", 0)) for mp in plan.mps]}


def position_codes(acts, position):
    """The codes at ``position`` of a plan_activations / "activations" dict, flattened."""
    if position == "predict":
        return list(acts["predict"])
    if position == "readout_op":
        return [c for op in acts["readout_ops"] for c in op]
    if position == "message":
        return [c for mp in acts["message"] for net in mp for c in net]
    return list(acts["convolution"])


def no_normalization(desc):
    """Features taken as given (tests/shape_cases.py's builders draw them in [-1, 1))."""
    d = copy.deepcopy(desc)
    for e in d["entities"]:
        for f in e["features"]:
            f["normalization"] = "None"
    return d


# ---------------------------------------------------------------------------------------------
# forward cases: one position x one name on the P sweep's graphs of 1, 15, 16, 17 and 129 path rows
ROWS = (1, 15, 16, 17, 129)
FORWARD_POSITIONS = {
    # position: (model, the tensors of the layer under test)
    "hidden": (lambda n: predict_model(n, 0, widths=(32, 1), acts=("selu", "None")), "readout_model_0/predict_0/"),
    "hidden16": (lambda n: predict_model(n, 0, widths=(16, 1), acts=("selu", "None")), "readout_model_0/predict_0/"),
    "act3": (lambda n: predict_model(n, 2), "readout_model_0/predict_2/"),
    "readout_op": (readout_op_model, "readout_model_0/layer_0_Dense_readout/"),
    "message": (message_model, "path_to_link_message_creation_0/layer_0_Dense_message_creation_0/"),
    "message_last": (message_last_model, "path_to_link_message_creation_0/layer_1_Dense_message_creation_0/"),
    "convolution": (conv_model, "convolution/"),
}
# The standard deviation the layer's pre-activations are centred and scaled to (scale_layer), so
# that REGIMES below hold: elu's kink, hard_sigmoid's two saturations, softplus' two tails
TARGET_STD = {"elu": 1.0, "softplus": 10.0, "softsign": 2.0, "exponential": 3.0, "hard_sigmoid": 4.0}
REGIMES = {
    "elu": [lambda z: z < -0.25, lambda z: np.abs(z) <= 0.25, lambda z: z > 0.25],
    "softplus": [lambda z: z < -8, lambda z: np.abs(z) <= 8, lambda z: z > 8],
    "softsign": [lambda z: z < 0, lambda z: z > 0],
    "exponential": [lambda z: z < 0, lambda z: z > 0],
    "hard_sigmoid": [lambda z: z < -2.5, lambda z: np.abs(z) <= 2.5, lambda z: z > 2.5],
}


def check_regimes(name, z):
    """Each regime of ``name`` holds at least a tenth of the oracle's pre-activations z: a condition on
    the inputs."""
    z = np.concatenate([np.asarray(x).reshape(-1) for x in z])
    frac = [float(r(z).mean()) for r in REGIMES[name]]
    assert min(frac) >= 0.1, "%s: regime fractions %s over %d pre-activations" % (name, frac, z.size)
    if name == "softplus":
        assert 15 <= np.abs(z).max() <= 60, np.abs(z).max()
    if name == "exponential":   # exp(z) and what follows it stay far inside float32
        assert np.abs(z).max() <= 30, np.abs(z).max()
    return frac


def scale_layer(prm, prefix, factor, shift=0.0):
    """The layer's kernel x factor and its bias -> (bias - shift) x factor: pre-activations z -> (z - shift) x factor."""
    out = dict(prm)
    for k in prm:
        if k.startswith(prefix):
            v = np.asarray(prm[k], np.float64) - (shift if k.endswith("/bias") else 0.0)
            out[k] = (v * factor).astype(np.float32)
    return out


def forward_case(position, name, seen, rows=ROWS):
    """(description, dims, plan, graphs, parameters, float64 reference per graph, IEEE float32 evaluation
    per graph) with the layer under test scaled to TARGET_STD[name] and check_regimes asserted on the
    oracle's pre-activations.  ``seen``: the new_activations fixture's list."""
    from oracle.dense_forward import DenseOracle
    from tests import shape_cases as sc
    model, prefix = FORWARD_POSITIONS[position]
    desc, dims = no_normalization(model(name)), sc.dims("routenet")
    graphs = [sc.graph(sc.P_GRAPH[p]) for p in rows]
    _, plan, _, prm = sc.inputs_for(desc, dims, graphs)
    del seen[:]
    DenseOracle(desc, dims, prm).forward(graphs)
    z0 = np.concatenate(seen)   # centred (where the layer has a bias) and scaled to the target
    prm = scale_layer(prm, prefix, TARGET_STD[name] / z0.std(), z0.mean())
    del seen[:]
    ref = [DenseOracle(desc, dims, prm).forward([g]) for g in graphs]
    check_regimes(name, seen)
    with np.errstate(over="ignore"):
        ieee = [DenseOracle(desc, dims, prm, dtype=np.float32).forward([g]) for g in graphs]
    return desc, dims, plan, graphs, prm, ref, ieee


# each forward position's key in NAMES_AT
FORWARD_AT = {"hidden": "predict", "hidden16": "predict", "act3": "predict", "readout_op": "readout_op",
              "message": "message", "message_last": "message", "convolution": "convolution"}
