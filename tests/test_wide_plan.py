"""Plans with 128-wide GRU cells (CPU): they lower through MPPlan -> ign_plan_create and through
ign_plan_create_json to the same plan, and what stays refused at 128 is refused by both in the same words."""
import copy
import ctypes as C

import pytest

from ignnition_amd import _lib, model_examples as me
from ignnition_amd.engine import MPPlan
from ignnition_amd.json_operations import Model_information
from tests import wide_cases as wc
from tests.test_plan_json import QSIZE_DIMS, ROUTENET_DIMS, _create_json, _describe, _tensors, _widths


def _python_plan(desc, dims):
    """(status, handle, error text, MPPlan) of the Python lowering's plan, cell options included."""
    plan = MPPlan.from_model_info(Model_information(copy.deepcopy(desc), dims))
    d, keep = plan.to_desc()
    h = C.c_void_p()
    rc = _lib.lib.ign_plan_create(C.byref(d), 0, C.byref(h))
    try:
        if rc == 0:
            plan.set_cell_options(h)
    except _lib.EngineError as e:
        _lib.lib.ign_plan_destroy(h)
        rc, h = e.code, None
    return rc, h, _lib.lib.ign_last_error().decode(), plan


@pytest.mark.parametrize("kind", ["routenet", "qsize", "concat1"])
def test_wide_models_lower_alike(kind):
    desc, dims = wc.model(kind)
    rc, hp, err, plan = _python_plan(desc, dims)
    assert rc == 0, err
    rc, hj = _create_json(desc, dims)
    try:
        assert rc == 0, _lib.lib.ign_last_error()
        tensors, total = _tensors(hj)
        assert (tensors, total) == _tensors(hp)
        info, specs = _describe(hj), plan.param_specs()
        assert [(p["name"], tuple(p["shape"])) for p in info["params"]] == [(n, tuple(s)) for n, s in specs]
        assert [e["hidden"] for e in info["entities"]] == plan.hidden == [128] * len(plan.entities)
    finally:
        _lib.lib.ign_plan_destroy(hp)
        if hj:
            _lib.lib.ign_plan_destroy(hj)


def _no_reset_after(desc):
    [n for n in desc["neural_networks"] if n["nn_name"] == "recurrent1"][0]["reset_after"] = False
    return desc


_ONLY = "a 128-wide GRU cell takes 128-wide messages only "
REFUSED = {
    "attention": (me.routenet_aggregation({"type": "attention"}, hidden=128), ROUTENET_DIMS,
                  "mp 1: attention / convolution lowered for 16 or 32 units"),
    "convolution": (me.routenet_aggregation({"type": "convolution"}, hidden=128), ROUTENET_DIMS,
                    "mp 1: attention / convolution lowered for 16 or 32 units"),
    "concat2": (me.qsize_aggregation({"type": "concat", "concat_axis": 2}, hidden=128), QSIZE_DIMS,
                "mp 0: concat on axis 2 is not lowered at 128 units (slice 128, units 128)"),
    "link32_path128": (_widths(me.routenet(), link=32, path=128), ROUTENET_DIMS, "mp 0: " + _ONLY + "(input 32, units 128)"),
    "message_net_32": (me.routenet_message_net(units=(32,), hidden=128), ROUTENET_DIMS,
                       "mp 1: " + _ONLY + "(input 32, units 128)"),
    "cell_options": (_no_reset_after(me.routenet(hidden=128)), ROUTENET_DIMS,
                     "is 128 units wide: a GRU cell with options is lowered at 16, 32 and 64 units"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_at_128(case):
    desc, dims, text = REFUSED[case]
    rc, hp, from_python, _ = _python_plan(desc, dims)
    assert rc == -2 and not hp and text in from_python, from_python
    rc, hj = _create_json(desc, dims)
    assert rc == -2 and not hj and _lib.lib.ign_last_error().decode() == from_python
