"""elu, softplus, softsign, exponential and hard_sigmoid in the plan lowerings (CPU, no GPU): both front
ends (engine.MPPlan and ign_plan_create_json) carry the same activation code in every position a model
description can name one; swish, softmax, an unknown name and the position / name pairs that existing tests
pin (activation_cases.REFUSED_AT) are refused by both with the same status and text; and tests/activation_cases.py's restatements agree with finite differences."""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch

from ignnition_amd import _lib
from ignnition_amd.engine import MPPlan, UnsupportedModel
from ignnition_amd.json_operations import Model_information
from tests import activation_cases as ac
from tests.test_plan_json import ROUTENET_DIMS, _create_json, _describe, _tensors

CASES = [(pos, name) for pos in ac.POSITIONS for name in ac.NAMES_AT[pos]]


def test_codes_are_the_abi_values():
    assert _lib.ACT["tanh"] == 4 and {n: _lib.ACT[n] for n in ac.NAMES} == ac.CODES
    assert _lib.lib.ign_abi_version() == 13   # additive enum values, no struct change


@pytest.mark.parametrize("position,name", CASES)
def test_both_front_ends_lower_the_code(position, name):
    desc = ac.POSITIONS[position](name)
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), ROUTENET_DIMS))
    acts = ac.plan_activations(plan)
    assert ac.CODES[name] in ac.position_codes(acts, position), acts
    d, keep = plan.to_desc()
    hp = C.c_void_p()
    rc = _lib.lib.ign_plan_create(C.byref(d), 0, C.byref(hp))
    assert rc == 0, _lib.lib.ign_last_error()
    rc, hj = _create_json(desc, ROUTENET_DIMS)
    try:
        assert rc == 0, _lib.lib.ign_last_error()
        assert _describe(hj)["activations"] == acts
        assert _tensors(hj) == _tensors(hp)
    finally:
        _lib.lib.ign_plan_destroy(hp)
        if hj:
            _lib.lib.ign_plan_destroy(hj)


@pytest.mark.parametrize("position,name", [(p, n) for p in ac.POSITIONS for n in ac.REFUSED + ac.REFUSED_AT[p]])
def test_refused_by_name_in_both_front_ends(position, name):
    """swish, softmax, an unknown name, and the pairs existing tests pin as refused (activation_cases.REFUSED_AT)."""
    desc = ac.POSITIONS[position](name)
    with pytest.raises(UnsupportedModel) as e:
        MPPlan.from_model_info(Model_information(copy.deepcopy(desc), ROUTENET_DIMS))
    rc, hj = _create_json(desc, ROUTENET_DIMS)
    assert rc == -2 and not hj   # IGN_ERR_UNSUPPORTED, UnsupportedModel's status
    text = _lib.lib.ign_last_error().decode()
    assert "activation '%s' not supported" % name in text
    assert str(e.value) in text


# points away from the kinks (0 for elu, +-2.5 for hard_sigmoid) by more than the difference step
Z = np.array([-19.3, -6.1, -2.9, -2.1, -0.7, -0.01, 0.013, 0.4, 1.9, 2.2, 3.1, 7.7, 18.6])
H = 1e-6


@pytest.mark.parametrize("name", ac.NAMES)
def test_restatements_against_finite_differences(name):
    """d act / dz by a centred difference in float64 = torch autograd of the torch restatement = grad_out of
    the activation's output; the numpy and torch restatements agree, and float32 stays float32."""
    fd = (ac.act_np(Z + H, name) - ac.act_np(Z - H, name)) / (2 * H)
    a = ac.act_np(Z, name)
    scale = np.maximum(np.abs(fd), 1e-300)
    assert np.all(np.abs(ac.grad_out(a, name) - fd) <= 1e-8 * scale + 1e-9 * np.abs(a) + 1e-15)
    zt = torch.tensor(Z, dtype=torch.float64, requires_grad=True)
    at = ac.act_torch(zt, name)
    np.testing.assert_allclose(at.detach().numpy(), a, rtol=1e-14, atol=0)
    at.sum().backward()
    np.testing.assert_allclose(zt.grad.numpy(), ac.grad_out(a, name), rtol=1e-12, atol=0)
    assert ac.act_np(Z.astype(np.float32), name).dtype == np.float32


def test_softplus_tails_do_not_cancel():
    """softplus(-19.3) = 4.1e-9 and its derivative through that output, to full precision: the forms the
    engine must keep (max(z, 0) + log1p(exp(-|z|)), -expm1(-a))."""
    a = ac.act_np(np.array([-19.3]), "softplus")
    assert a[0] == pytest.approx(np.exp(-19.3), rel=1e-8)
    assert ac.grad_out(a, "softplus")[0] == pytest.approx(np.exp(-19.3), rel=1e-8)
    assert ac.act_np(np.array([800.0]), "softplus")[0] == 800.0


def test_oracles_take_the_names_only_under_the_fixture(new_activations):
    import oracle.dense_forward as dense
    import oracle.train_oracle as train
    x = np.array([[-1.0, 2.0]])
    np.testing.assert_array_equal(dense._act(x, "elu"), ac.act_np(x, "elu"))
    np.testing.assert_array_equal(dense._act(x, "relu"), np.maximum(x, 0))
    assert torch.equal(train._act(torch.tensor(x), "softsign"), ac.act_torch(torch.tensor(x), "softsign"))
    with pytest.raises(dense.OracleError):
        dense._act(x, "swish")


def test_abi_refuses_the_pinned_pairs():
    """ign_plan_create itself refuses them (a descriptor built past the front ends' name checks)."""
    for position, names in ac.REFUSED_AT.items():
        for name in names:
            plan = MPPlan.from_model_info(Model_information(ac.POSITIONS[position]("tanh"), ROUTENET_DIMS))
            if position == "readout_op":
                plan.readout_ops[0]["layers"] = [l[:2] + (ac.CODES[name],) + l[3:] for l in plan.readout_ops[0]["layers"]]
            elif position == "message":
                for mp in plan.mps:
                    for net in mp["nets"]:
                        if net:
                            net["layers"] = [l[:2] + (ac.CODES[name],) + l[3:] for l in net["layers"]]
            else:
                for mp in plan.mps:
                    if mp["aggr"] == "convolution":
                        mp["act"] = ac.CODES[name]
            d, keep = plan.to_desc()
            h = C.c_void_p()
            assert _lib.lib.ign_plan_create(C.byref(d), 0, C.byref(h)) == -2 and not h, (position, name)
            assert ("activation %d" % ac.CODES[name]) in _lib.lib.ign_last_error().decode()


new_activations = ac.new_activations
