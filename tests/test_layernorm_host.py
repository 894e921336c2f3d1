"""LayerNormalization in the readout's Dense stacks, the parts that need no GPU: the lowering of both
front ends (MPPlan and ign_plan_create_json): parameter names and shapes, the layers' records and
their order relative to Dropout, refusals; ign_plan_add_layernorm's argument checks; the checkpoint
round trip."""
import copy
import ctypes as C
import json

import numpy as np
import pytest

from ignnition_amd import _lib, checkpoint, model_examples, workloads
from ignnition_amd import framework_operations as fo
from ignnition_amd.engine import MPPlan, UnsupportedModel
from ignnition_amd.json_operations import Model_information
from tests import dropout_cases as dc
from tests import layernorm_cases as lc
from tests.layernorm_cases import drop, ln
from tests.predict_cases import predict_model

DIMS = workloads.model("routenet")[1]


def _create_json(desc):
    h = C.c_void_p()
    rc = _lib.lib.ign_plan_create_json(json.dumps(desc).encode(), json.dumps(DIMS).encode(), 0, C.byref(h))
    return rc, h, _lib.lib.ign_last_error().decode(errors="replace")


def _describe(h):
    need = C.c_int64()
    _lib.check(_lib.lib.ign_plan_describe_json(h, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _lib.check(_lib.lib.ign_plan_describe_json(h, buf, need.value, C.byref(need)))
    return json.loads(buf.value.decode())


def _plan(desc):
    return MPPlan.from_model_info(Model_information(copy.deepcopy(desc), DIMS))


def _unnamed(desc):
    for net in desc["neural_networks"]:
        for l in net.get("nn_architecture", []):
            l.pop("name", None)
    return desc


def _tensors(h):
    """[(kind, owner, offset, rows, cols)] of ign_plan_param_tensor."""
    nt = C.c_int32()
    _lib.check(_lib.lib.ign_plan_num_param_tensors(h, C.byref(nt)))
    out = []
    for i in range(nt.value):
        kind, owner, off, rows, cols = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32()
        _lib.check(_lib.lib.ign_plan_param_tensor(h, i, C.byref(kind), C.byref(owner), C.byref(off), C.byref(rows),
                                                  C.byref(cols)))
        out.append((kind.value, owner.value, off.value, rows.value, cols.value))
    return out


LOWERING = {
    "between": lambda: lc.ln_model("selu", [(1, ln())]),
    "first": lambda: lc.ln_model("odd_widths", [(0, ln(epsilon=1e-5))]),
    "last": lambda: lc.ln_model("odd_widths", [(3, ln(name="final_ln"))]),
    "ln_then_dropout": lambda: lc.ln_model("four_layer", [(1, ln()), (1, drop(0.5))]),
    "dropout_then_ln": lambda: lc.ln_model("four_layer", [(1, drop(0.5)), (1, ln())]),
    "readout_op": lc.pooled_model,
    "unnamed": lambda: _unnamed(lc.ln_model("four_layer", [(1, ln()), (3, drop(0.5)), (3, ln())])),
    "center_false": lambda: lc.ln_model("selu", [(1, ln(center=False))]),
    "scale_false": lambda: lc.ln_model("selu", [(2, ln(scale=False, axis=-1))]),
}


@pytest.mark.parametrize("case", sorted(LOWERING))
def test_both_front_ends_agree(case):
    desc = LOWERING[case]()
    plan = _plan(desc)
    rc, h, err = _create_json(desc)
    assert rc == 0, err
    try:
        doc = _describe(h)
        specs = plan.param_specs()
        assert [(p["name"], tuple(p["shape"])) for p in doc["params"]] == [(n, tuple(s)) for n, s in specs]
        sites = plan.layernorm_sites()
        assert len(sites) > 0
        assert [(d["site"], d["stack"], d["before_layer"], d["order"], np.float32(d["epsilon"]), d["center"], d["scale"],
                 d["units"], d["name"]) for d in doc["layernorm"]] == \
               [(s, st, b, o, np.float32(e), c, sc, u, n) for s, st, b, o, e, c, sc, u, n in sites]
        assert [(d["site"], d["stack"], d["before_layer"], np.float32(d["rate"]), d["seed"]) for d in doc["dropout"]] == \
               [(s, st, b, np.float32(r), sd) for s, st, b, r, sd in plan.dropout_sites()]
        # the engine's tensors: kinds 13 / 14 where the names say gamma / beta, with the names' shapes
        tensors = _tensors(h)
        assert len(tensors) == len(specs)
        for (name, shape), (kind, owner, _, rows, cols) in zip(specs, tensors):
            assert (kind == 13) == name.endswith("/gamma") and (kind == 14) == name.endswith("/beta"), name
            assert rows * cols == int(np.prod(shape)), name
            if kind in (13, 14):
                assert 0 <= owner < len(sites) and cols == sites[owner][7] and sites[owner][8] in name
        offs = [t[2] for t in tensors]
        assert offs == sorted(offs) and len(set(offs)) == len(offs)
    finally:
        _lib.lib.ign_plan_destroy(h)
    names = [n for n, _ in plan.param_specs()]
    by = {s[8]: s for s in sites}
    if case == "between":
        assert names[-8:] == ["readout_model_0/predict_0/kernel", "readout_model_0/predict_0/bias",
                              "readout_model_0/layer_1_LayerNormalization_readout/gamma",
                              "readout_model_0/layer_1_LayerNormalization_readout/beta",
                              "readout_model_0/predict_1/kernel", "readout_model_0/predict_1/bias",
                              "readout_model_0/predict_2/kernel", "readout_model_0/predict_2/bias"]
        assert sites == [(0, -1, 1, 0, 1e-3, True, True, 256, "layer_1_LayerNormalization_readout")]
    if case == "first":
        assert sites == [(0, -1, 0, 0, 1e-5, True, True, 32, "layer_0_LayerNormalization_readout")]
        assert names.index("readout_model_0/layer_0_LayerNormalization_readout/gamma") < names.index("readout_model_0/predict_0/kernel")
    if case == "last":
        assert sites == [(0, -1, 3, 0, 1e-3, True, True, 1, "final_ln")]
        assert names[-2:] == ["readout_model_0/final_ln/gamma", "readout_model_0/final_ln/beta"]
    if case == "ln_then_dropout":
        assert [(s[2], s[3]) for s in sites] == [(1, 0)] and [d[2] for d in plan.dropout_sites()] == [1]
        assert [c[0] for c in plan.stack_sites()] == ["layernorm", "dropout"]
    if case == "dropout_then_ln":
        assert [(s[2], s[3]) for s in sites] == [(1, 1)]
        assert [c[0] for c in plan.stack_sites()] == ["dropout", "layernorm"]
    if case == "readout_op":   # readout operations first, then predict
        assert [(s[1], s[2], s[7]) for s in sites] == [(0, 1, 24), (-1, 0, 16)]
        assert "readout_model_0/layer_1_LayerNormalization_readout/gamma" in names and "readout_model_2/ln_first/beta" in names
    if case == "unnamed":
        # Feed_forward_model numbers every layer: Dense, LN, Dense, Dense, Dropout, LN, Dense
        assert [n for n in names if n.startswith("readout_model_0/") and n.endswith("/kernel")] == [
            "readout_model_0/layer_%d_Dense_readout/kernel" % i for i in (0, 2, 3, 6)]
        assert [(s[2], s[3], s[8]) for s in sites] == [(1, 0, "layer_1_LayerNormalization_readout"),
                                                       (3, 1, "layer_5_LayerNormalization_readout")]
    if case == "center_false":
        assert by["layer_1_LayerNormalization_readout"][5:7] == (False, True)
        assert not any(n.endswith("/beta") for n in names) and sum(n.endswith("/gamma") for n in names) == 1
    if case == "scale_false":
        assert by["layer_2_LayerNormalization_readout"][5:7] == (True, False)
        assert not any(n.endswith("/gamma") for n in names) and sum(n.endswith("/beta") for n in names) == 1


def test_init_params_gamma_ones_beta_zeros():
    plan = _plan(LOWERING["between"]())
    prm = plan.init_params(0)
    g = "readout_model_0/layer_1_LayerNormalization_readout/"
    assert prm[g + "gamma"].shape == (256,) and (prm[g + "gamma"] == 1).all() and (prm[g + "beta"] == 0).all()


def _refused(desc, text, code=-2, exc=UnsupportedModel):
    with pytest.raises(exc) as e:
        _plan(desc)
    assert text in str(e.value)
    rc, _, err = _create_json(desc)
    assert rc == code and text in err
    return str(e.value), err


def test_unknown_option_is_unsupported():
    for key, value in (("beta_initializer", "ones"), ("gamma_regularizer", 0.1), ("beta_constraint", "non_neg")):
        a, b = _refused(lc.ln_model("selu", [(1, ln(**{key: value}))]), "LayerNormalization option '%s' is not lowered" % key)
        assert a == b == "LayerNormalization option '%s' is not lowered" % key


def test_axis_zero_is_unsupported():
    a, b = _refused(lc.ln_model("selu", [(1, ln(axis=0))]), "axis")
    assert a == b
    c, d = _refused(lc.ln_model("selu", [(1, ln(axis=0.0))]), "axis")   # a float that holds an integer: the same
    assert c == d == a
    for axis in (-1, 1, 1.0, -1.0):
        assert _plan(lc.ln_model("selu", [(1, ln(axis=axis))])).layernorm_sites()[0][2] == 1
        rc, h, err = _create_json(lc.ln_model("selu", [(1, ln(axis=axis))]))
        assert rc == 0, err
        _lib.lib.ign_plan_destroy(h)


def test_negative_epsilon_is_invalid():
    desc = lc.ln_model("selu", [(1, ln(epsilon=-1e-3))])
    with pytest.raises(ValueError) as e:
        _plan(desc)
    assert not isinstance(e.value, UnsupportedModel) and "epsilon" in str(e.value)
    rc, _, err = _create_json(desc)
    assert rc == -1 and "epsilon" in err   # IGN_ERR_INVALID


def test_layernorm_in_a_message_network_is_unsupported():
    desc = model_examples.routenet_message_net(units=(24, 32), iterations=3)
    for net in desc["neural_networks"]:
        if net["nn_name"] == "message_nn":
            net["nn_architecture"].insert(1, ln())
    a, b = _refused(desc, "message layer type LayerNormalization is not lowered (Dense only)")
    assert a == b == "message layer type LayerNormalization is not lowered (Dense only)"


def test_other_layer_types_name_the_three_lowered():
    desc = lc.ln_model("selu", [(1, {"type_layer": "BatchNormalization"})])
    a, b = _refused(desc, "readout layer type BatchNormalization is not lowered (Dense, Dropout and LayerNormalization only)")
    assert a == b


def test_plan_without_the_layer_is_unchanged():
    """param_specs and to_desc of a description without the layer: the Dense tensors alone, in the
    order they had, and the same ign_plan_desc as the description with one (the layer is not in it)."""
    plain = _plan(predict_model("selu"))
    assert plain.layernorm_sites() == [] and plain.stack_sites() == []
    assert [n for n, _ in plain.param_specs()] == [
        "path_update/kernel", "path_update/recurrent_kernel", "path_update/bias",
        "link_update/kernel", "link_update/recurrent_kernel", "link_update/bias"] + [
        "readout_model_0/predict_%d/%s" % (i, t) for i in range(3) for t in ("kernel", "bias")]
    with_ln = _plan(lc.ln_model("selu", [(1, ln())]))
    a, _ = plain.to_desc()
    b, _ = with_ln.to_desc()
    assert a.num_dense == b.num_dense == 3
    assert [(a.dense[i].units, a.dense[i].activation) for i in range(3)] == [(b.dense[i].units, b.dense[i].activation) for i in range(3)]
    assert [s for s in with_ln.param_specs() if "LayerNormalization" not in s[0]] == plain.param_specs()
    # the engine's layout of the plain plan: no tensor of kind 13 / 14, and the JSON front end's equal to it
    h = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create(C.byref(a), 0, C.byref(h)))
    rc, hj, err = _create_json(predict_model("selu"))
    assert rc == 0, err
    try:
        assert _tensors(h) == _tensors(hj) and not any(t[0] in (13, 14) for t in _tensors(h))
        assert _describe(hj)["layernorm"] == []
    finally:
        _lib.lib.ign_plan_destroy(h)
        _lib.lib.ign_plan_destroy(hj)


def test_add_layernorm_arguments_and_order():
    """ign_plan_add_layernorm on a plan from ign_plan_create: argument checks, the tensors it adds, and
    refused once ign_batch_create was called on the plan."""
    plan = _plan(dc.readout_op_model())   # op 0: two Dense layers (24, 16); op 1: pooling; predict: (64, 1)
    desc, keep = plan.to_desc()
    h = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create(C.byref(desc), 0, C.byref(h)))
    try:
        add = _lib.lib.ign_plan_add_layernorm
        before = _tensors(h)
        assert add(h, -1, 3, 1e-3, 1, 1) == -1      # predict has two layers
        assert add(h, 1, 0, 1e-3, 1, 1) == -1       # the pooling operation has no Dense stack
        assert add(h, 5, 0, 1e-3, 1, 1) == -1
        assert add(h, -2, 0, 1e-3, 1, 1) == -1
        assert add(h, -1, 0, -1e-3, 1, 1) == -1
        assert "epsilon" in _lib.lib.ign_last_error().decode()
        assert add(h, -1, 0, float("nan"), 1, 1) == -1
        assert _tensors(h) == before                 # a refused call changes nothing
        assert add(h, -1, 2, 1e-3, 1, 1) == 0       # after the last of predict's two layers: width 1
        assert add(h, -1, 1, 0.0, 0, 1) == 0        # gamma alone, width 64
        assert add(h, 0, 1, 1e-5, 1, 0) == 0        # beta alone, width 24, in operation 0
        assert add(h, -1, 0, 1e-3, 0, 0) == 0       # no tensor at all
        after = _tensors(h)
        plain = [t for t in after if t[0] not in (13, 14)]
        assert [(t[0], t[1], t[3], t[4]) for t in plain] == [(t[0], t[1], t[3], t[4]) for t in before]
        # in layout order: op 0's beta (site 0) in front of its layer 1, then predict's gamma (site 2)
        # in front of layer 1, and gamma, beta (site 3) at the end
        assert [(t[0], t[1], t[4]) for t in after if t[0] in (13, 14)] == [(14, 0, 24), (13, 2, 64), (13, 3, 1), (14, 3, 1)]
        kinds = [t[0] for t in after]
        assert kinds[kinds.index(14) - 1:kinds.index(14) + 2] == [12, 14, 11]
        bd = _lib.BatchDesc()                        # an empty description: the call fails, and closes the layer list
        b = C.c_void_p()
        assert _lib.lib.ign_batch_create(h, C.byref(bd), C.byref(b)) != 0
        assert add(h, -1, 1, 1e-3, 1, 1) == -1
        assert "batch" in _lib.lib.ign_last_error().decode()
        assert _tensors(h) == after
    finally:
        _lib.lib.ign_plan_destroy(h)


def test_checkpoint_round_trip_keeps_gamma_and_beta(tmp_path):
    plan = _plan(lc.pooled_model())
    prm = plan.init_params(5, bias_scale=0.3)
    ln_names = [n for n in prm if n.endswith("/gamma") or n.endswith("/beta")]
    assert len(ln_names) == 4
    for n in ln_names:
        assert np.ptp(prm[n]) > 0
    path = str(tmp_path / "ckpt.safetensors")
    checkpoint.save_params(prm, path)
    back = checkpoint.load_params(path)
    assert list(back) and set(back) == set(prm) == {n for n, _ in plan.param_specs()}
    for (n, shape) in plan.param_specs():
        assert back[n].shape == tuple(shape) and back[n].dtype == np.float32
        np.testing.assert_array_equal(back[n], prm[n])
    # the reference's warm-start patterns select kernels and biases only, as in TF
    warm = fo.warm_start(plan.init_params(0), back)
    for n in ln_names:
        np.testing.assert_array_equal(warm[n], plan.init_params(0)[n])
    assert np.array_equal(warm["readout_model_2/predict_0/kernel"], back["readout_model_2/predict_0/kernel"])


def test_debug_dump_lists_the_layers(tmp_path):
    mi = Model_information(lc.ln_model("selu", [(1, ln(epsilon=1e-5, center=False))]), DIMS)
    dump = fo.debug(mi, str(tmp_path))
    assert dump["layernorm_sites"] == [{"site": 0, "stack": -1, "before_layer": 1, "order": 0, "epsilon": 1e-5,
                                        "center": False, "scale": True, "units": 256,
                                        "name": "layer_1_LayerNormalization_readout"}]
    assert ["readout_model_0/layer_1_LayerNormalization_readout/gamma", [256]] in dump["parameters"]
