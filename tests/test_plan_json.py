"""ign_plan_create_json (CPU, no GPU): the C++ lowering of model_description.json + dimensions
gives the same plan as the Python path (Model_information -> MPPlan.to_desc -> ign_plan_create):
the same parameter tensors (kind, owner, offset, shape), the same Keras-style names, adjacency /
interleave input keys and entity order, and the same errors for models the engine or the
reference rejects (JO:184-245, GM:338, AUX:764)."""
import copy
import ctypes as C
import json

import pytest

from ignnition_amd import _lib, model_examples, workloads
from ignnition_amd.engine import MPPlan
from ignnition_amd.json_operations import Model_information
from tests.predict_cases import PREDICT_CASES, SATURATED, predict_model
from tests.readout_cases import READOUT_CASES
from tests.width_cases import CASES as WIDTH_FEATURE_CASES

ROUTENET_DIMS = workloads.model("routenet")[1]
QSIZE_DIMS = workloads.model("qsize")[1]
SYNTH_DIMS = {"node_feature": 1, "target": 1, "entities": 0, "adj_nodes_nodes": 0}


def _cases():
    c = {"routenet": (model_examples.routenet(), ROUTENET_DIMS),
         "routenet_h16_t3": (model_examples.routenet(hidden=16, iterations=3), ROUTENET_DIMS),
         "qsize": (model_examples.qsize(), QSIZE_DIMS),
         "synthetic": (model_examples.synthetic_graph(), SYNTH_DIMS)}
    for a in ({"type": "attention"}, {"type": "convolution", "activation_function": "tanh"}, {"type": "ordered"}):
        c["routenet_" + a["type"]] = (model_examples.routenet_aggregation(a), ROUTENET_DIMS)
    for a in ({"type": "attention"}, {"type": "convolution"}, {"type": "concat", "concat_axis": 1},
              {"type": "concat", "concat_axis": 2}):
        c["qsize_%s%s" % (a["type"], a.get("concat_axis", ""))] = (model_examples.qsize_aggregation(a), QSIZE_DIMS)
    c["routenet_msgnet"] = (model_examples.routenet_message_net(inputs=("hs_source", "hs_dest"), units=(24, 32),
                                                                activation="selu"), ROUTENET_DIMS)
    for name, (ops, pin, nets) in READOUT_CASES.items():
        c["readout_" + name] = (model_examples.routenet_readout(ops, pin, nets), ROUTENET_DIMS)
    # predict networks: use_bias false, the four activation strings and "None", 1 to 4 layers, odd widths
    for name in PREDICT_CASES:
        if name not in SATURATED:   # (the same descriptions as relu / selu / tanh / sigmoid)
            c["predict_" + name] = (predict_model(name), ROUTENET_DIMS)
    # unequal entity widths, axis-2 slices of different widths, features of several columns
    for name, build in WIDTH_FEATURE_CASES.items():
        c["width_" + name] = build()[:2]
    return c


CASES = _cases()


def _tensors(h):
    n = C.c_int32()
    _lib.check(_lib.lib.ign_plan_num_param_tensors(h, C.byref(n)))
    out = []
    for i in range(n.value):
        k, o, off, r, c = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32()
        _lib.check(_lib.lib.ign_plan_param_tensor(h, i, C.byref(k), C.byref(o), C.byref(off), C.byref(r), C.byref(c)))
        out.append((k.value, o.value, off.value, r.value, c.value))
    total = C.c_int64()
    _lib.check(_lib.lib.ign_plan_num_params(h, C.byref(total)))
    return out, total.value


def _create_json(desc, dims):
    h = C.c_void_p()
    rc = _lib.lib.ign_plan_create_json(json.dumps(desc).encode(), json.dumps(dims).encode(), 0, C.byref(h))
    return rc, h


def _describe(h):
    need = C.c_int64()
    _lib.check(_lib.lib.ign_plan_describe_json(h, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _lib.check(_lib.lib.ign_plan_describe_json(h, buf, need.value, C.byref(need)))
    return json.loads(buf.value.decode())


@pytest.mark.parametrize("case", sorted(CASES))
def test_json_plan_equals_python_lowering(case):
    desc, dims = CASES[case]
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    d, keep = plan.to_desc()
    hp = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create(C.byref(d), 0, C.byref(hp)))
    rc, hj = _create_json(desc, dims)
    try:
        assert rc == 0, _lib.lib.ign_last_error()
        assert _tensors(hj) == _tensors(hp)
        info = _describe(hj)
        specs = plan.param_specs()
        assert [p["name"] for p in info["params"]] == [n for n, _ in specs]
        assert [tuple(p["shape"]) for p in info["params"]] == [tuple(s) for _, s in specs]
        assert [e["name"] for e in info["entities"]] == plan.entities
        assert [e["hidden"] for e in info["entities"]] == plan.hidden
        assert [[tuple(f) for f in e["features"]] for e in info["entities"]] == [list(f) for f in plan.features]
        assert [tuple(a["keys"]) for a in info["adjacencies"]] == [s.keys for s in plan.adj_slots]
        assert info["interleave"] == plan.il_slots
        assert info["label"] == plan.readout_label and info["iterations"] == plan.iterations
    finally:
        _lib.lib.ign_plan_destroy(hp)
        if hj:
            _lib.lib.ign_plan_destroy(hj)


def test_describe_needs_a_json_plan():
    plan = MPPlan.from_model_info(Model_information(model_examples.routenet(), ROUTENET_DIMS))
    d, keep = plan.to_desc()
    h = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create(C.byref(d), 0, C.byref(h)))
    try:
        assert _lib.lib.ign_plan_describe_json(h, None, 0, None) == -1
    finally:
        _lib.lib.ign_plan_destroy(h)


def _rejected(desc, dims, code, text):
    rc, h = _create_json(desc, dims)
    if h:
        _lib.lib.ign_plan_destroy(h)
    assert rc == code
    assert text in _lib.lib.ign_last_error().decode()


def test_unsupported_models_rejected_like_python():
    d = model_examples.routenet()
    d["message_passing"]["stages"][0]["stage_mp"][0]["update"] = {"type": "neural_network", "nn_name": "readout_model"}
    _rejected(d, ROUTENET_DIMS, -2, "GM:338")
    d = model_examples.routenet()
    for n in d["neural_networks"]:
        if n["nn_name"] == "recurrent1":
            n["recurrent_type"] = "LSTM"
    _rejected(d, ROUTENET_DIMS, -2, "AUX:764")
    d = model_examples.routenet()
    d["readout"][0]["input"] = ["link_capacity"]
    _rejected(d, ROUTENET_DIMS, -2, "raw input features")
    d = model_examples.routenet()
    d["readout"] = [{"type": "product", "type_product": "dot_product", "input": ["path", "path"], "output_name": "p"}] \
        + d["readout"]
    _rejected(d, ROUTENET_DIMS, -2, "tensordot")


def _widths(desc, **hidden):
    for e in desc["entities"]:
        e["hidden_state_dimension"] = hidden[e["name"]]
    return desc


def _refused_shapes():
    """{name: (desc, dims, status, message)}: entity widths and feature sizes the engine has no kernel
    for (IGN_ERR_UNSUPPORTED, -2) or that the reference's graph cannot be built with (IGN_ERR_INVALID, -1)."""
    c = {}
    for link, path in ((32, 64), (64, 32), (16, 64)):   # path <- link is (input link, units path)
        c["gru_l%d_p%d" % (link, path)] = (_widths(model_examples.routenet(), link=link, path=path), ROUTENET_DIMS, -2,
                                            "mp 0: GRU shape (input %d, units %d) not instantiated" % (link, path))
    c["interleave_l16_n32"] = (_widths(model_examples.qsize(), link=16, node=32, path=32), QSIZE_DIMS, -1,
                               "mp 0: sources have different message dimensions (16 vs 32)")
    for aggr in ("attention", "convolution"):
        c[aggr + "_p32_l16"] = (_widths(model_examples.routenet_aggregation({"type": aggr}), link=16, path=32),
                                ROUTENET_DIMS, -1, "mp 1: %s needs message dim 32 == destination dim 16" % aggr)
    c["concat2_slice64"] = (_widths(model_examples.qsize_aggregation({"type": "concat", "concat_axis": 2}), link=64,
                                    node=32, path=32), QSIZE_DIMS, -2,
                            "mp 0: concat slice (input 64, units 32) not instantiated")
    c["features_17_of_16"] = (model_examples.routenet(hidden=16), dict(ROUTENET_DIMS, link_capacity=17), -1,
                              "entity 0: total feature size 17 exceeds hidden_state_dimension 16")
    return c


REFUSED = _refused_shapes()


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_widths_and_feature_sizes(case):
    """ign_plan_create (the Python lowering's descriptor) and ign_plan_create_json refuse the shape with
    the same status and the same message; neither leaves a plan behind."""
    desc, dims, code, text = REFUSED[case]
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    d, keep = plan.to_desc()
    hp = C.c_void_p()
    rc = _lib.lib.ign_plan_create(C.byref(d), 0, C.byref(hp))
    from_python = _lib.lib.ign_last_error().decode()
    assert rc == code and not hp, from_python
    assert text in from_python
    rc, hj = _create_json(desc, dims)
    from_json = _lib.lib.ign_last_error().decode()
    assert rc == code and not hj, from_json
    assert from_json == from_python


@pytest.mark.parametrize("layer", [0, 2])
@pytest.mark.parametrize("act", ["gelu", "SELU", "softmax"])
def test_unknown_predict_activation_rejected(layer, act):
    """An activation name outside _lib.ACT in the predict network: UnsupportedModel from the Python
    lowering, IGN_ERR_UNSUPPORTED naming the activation from the C++ one (no silent linear layer)."""
    from ignnition_amd.engine import UnsupportedModel
    assert act not in _lib.ACT
    d = predict_model("selu")
    net = [n for n in d["neural_networks"] if n["nn_name"] == "readout_model"][0]
    net["nn_architecture"][layer]["activation"] = act
    with pytest.raises(UnsupportedModel, match="activation %r not supported" % act):
        MPPlan.from_model_info(Model_information(copy.deepcopy(d), ROUTENET_DIMS))
    _rejected(d, ROUTENET_DIMS, -2, "activation '%s' not supported" % act)


def test_reference_validation_errors():
    d = model_examples.routenet()
    d["message_passing"]["stages"][0]["stage_mp"][0]["source_entities"][0]["name"] = "router"
    _rejected(d, ROUTENET_DIMS, -1, "The source entity router was used in a message passing")
    d = model_examples.routenet()
    d["readout"][0]["nn_name"] = "nope"
    _rejected(d, ROUTENET_DIMS, -1, "The name nope is used as a reference to a neural network")
    dims = dict(ROUTENET_DIMS)
    dims.pop("traffic")
    _rejected(model_examples.routenet(), dims, -1, "no entry for 'traffic'")
    _rejected(model_examples.routenet(), {"a": 1}, -1, "no entry")
    rc, h = C.c_int(0), C.c_void_p()
    assert _lib.lib.ign_plan_create_json(b"{not json", b"{}", 0, C.byref(h)) == -1
    assert b"malformed model_description.json" in _lib.lib.ign_last_error()
