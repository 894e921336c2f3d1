"""Dropout in the readout's Dense stacks, the parts that need no GPU: the mask function
(ignnition_amd/csrc/dropout_rng.h) as a stand-alone g++ program, plain and sanitized;
ign_dropout_keep against a numpy restatement; the lowering of both front ends (MPPlan and
ign_plan_create_json): sites, rates, parameter names, refusals."""
import copy
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from ignnition_amd import _lib, model_examples, workloads
from ignnition_amd.engine import MPPlan, UnsupportedModel, dropout_keep
from ignnition_amd.json_operations import Model_information
from tests import dropout_cases as dc
from tests.predict_cases import predict_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = workloads.model("routenet")[1]
# the seeds the mask tests use: keep_numpy alone meets the cap below for each of them (checked
# before they were written here, and again by test_keep_fraction_of_the_restatement)
SEEDS = (0x299F31D0A4093822, 7)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_dropout_check(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the mask check"
    exe = str(tmp_path / "dropout_check")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tests", "cpp", "dropout_check.cpp"),
                         "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]


def test_numpy_restatement_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, out in kat:
        got = dc.philox4x32_10([np.array([c], np.uint64) for c in ctr], [np.array([k], np.uint64) for k in key])
        assert tuple(int(w[0]) for w in got) == out


@pytest.mark.parametrize("rows,units", [(1, 1), (182, 7), (364, 256)])
def test_keep_equals_numpy_restatement(rows, units):
    for rate in (0.25, 0.5):
        for seed in SEEDS:
            for site in (0, 3):
                for step in (0, 41):
                    np.testing.assert_array_equal(dropout_keep(seed, site, step, rows, units, rate),
                                                  dc.keep_numpy(seed, site, step, rows, units, rate))


def test_keep_fraction_of_the_restatement():
    """Sanity cap on (364, 256): |kept / n - (1 - rate)| <= 4 sqrt(rate (1 - rate) / n), for the
    restatement alone and so for ign_dropout_keep, which equals it."""
    n = 364 * 256
    for rate in (0.25, 0.5):
        for seed in SEEDS:
            for site in (0, 3):
                for step in (0, 41):
                    kept = int(dc.keep_numpy(seed, site, step, 364, 256, rate).sum())
                    assert abs(kept / n - (1 - rate)) <= 4 * math.sqrt(rate * (1 - rate) / n), (rate, seed, site, step)


def test_keep_arguments():
    out = np.zeros(4, np.uint8)
    p = out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert _lib.lib.ign_dropout_keep(1, 0, 0, 2, 2, C.c_float(1.0), p) == -1     # IGN_ERR_INVALID
    assert _lib.lib.ign_dropout_keep(1, 0, 0, 2, 2, C.c_float(-0.1), p) == -1
    assert _lib.lib.ign_dropout_keep(1, 0, 0, 2, 2, C.c_float(0.0), p) == 0
    assert out.tolist() == [1, 1, 1, 1]                                          # rate 0 keeps everything
    assert dropout_keep(1, 0, 0, 0, 5, 0.5).shape == (0, 5)


# ------------------------------------------------------------------------------------------ lowering
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


LOWERING = {
    "between": lambda: dc.dropout_model("selu", [(1, 0.5, {})]),
    "first_and_last": lambda: dc.dropout_model("odd_widths", [(0, 0.25, {"seed": 9}), (3, 0.5, {"name": "final_drop"})]),
    "adjacent": lambda: dc.dropout_model("four_layer", [(1, 0.5, {}), (1, 0.25, {"seed": 2}), (3, 0.5, {})]),
    "rate_zero": lambda: dc.dropout_model("two_layer", [(1, 0.0, {}), (2, 0.5, {})]),
    "unnamed": lambda: _unnamed(dc.dropout_model("four_layer", [(1, 0.5, {}), (3, 0.5, {})])),
    "readout_op": dc.readout_op_model,
}


@pytest.mark.parametrize("case", sorted(LOWERING))
def test_both_front_ends_agree(case):
    desc = LOWERING[case]()
    plan = _plan(desc)
    rc, h, err = _create_json(desc)
    assert rc == 0, err
    try:
        doc = _describe(h)
        assert [(p["name"], tuple(p["shape"])) for p in doc["params"]] == [(n, tuple(s)) for n, s in plan.param_specs()]
        sites = plan.dropout_sites()
        assert len(sites) > 0
        assert [(d["site"], d["stack"], d["before_layer"], np.float32(d["rate"]), d["seed"]) for d in doc["dropout"]] == \
               [(s, st, b, np.float32(r), sd) for s, st, b, r, sd in sites]
    finally:
        _lib.lib.ign_plan_destroy(h)
    names = [n for n, _ in plan.param_specs()]
    assert not any("Dropout" in n for n in names)   # a Dropout owns no parameters
    if case == "unnamed":
        # Feed_forward_model numbers every layer: Dense, Dropout, Dense, Dense, Dropout, Dense
        assert [n for n in names if n.startswith("readout_model_0/") and n.endswith("/kernel")] == [
            "readout_model_0/layer_%d_Dense_readout/kernel" % i for i in (0, 2, 3, 5)]
        assert [(b, r) for _, _, b, r, _ in sites] == [(1, 0.5), (3, 0.5)]
    if case == "adjacent":
        assert [(s, st, b, r, sd) for s, st, b, r, sd in sites] == [(0, -1, 1, 0.5, 0), (1, -1, 1, 0.25, 2), (2, -1, 3, 0.5, 0)]
    if case == "rate_zero":
        assert [(b, r) for _, _, b, r, _ in sites] == [(2, 0.5)]
    if case == "readout_op":   # readout operations first, then predict
        assert [(st, b, r, sd) for _, st, b, r, sd in sites] == [(0, 1, 0.5, 0), (0, 2, 0.25, 5)]
    if case == "first_and_last":
        assert [(b, r, sd) for _, _, b, r, sd in sites] == [(0, 0.25, 9), (3, 0.5, 0)]


def test_to_desc_is_unchanged_by_dropout():
    a, _ = _plan(predict_model("selu")).to_desc()
    b, _ = _plan(dc.dropout_model("selu", [(1, 0.5, {})])).to_desc()
    assert a.num_dense == b.num_dense == 3
    assert [(a.dense[i].units, a.dense[i].activation) for i in range(3)] == [(b.dense[i].units, b.dense[i].activation) for i in range(3)]


@pytest.mark.parametrize("rate", [-0.1, 1.0])
def test_rate_out_of_range_is_invalid(rate):
    desc = dc.dropout_model("selu", [(1, rate, {})])
    with pytest.raises(ValueError) as e:
        _plan(desc)
    assert not isinstance(e.value, UnsupportedModel) and "rate" in str(e.value)
    rc, _, err = _create_json(desc)
    assert rc == -1 and "rate" in err   # IGN_ERR_INVALID


def test_noise_shape_is_unsupported():
    desc = dc.dropout_model("selu", [(1, 0.5, {"noise_shape": [1, 256]})])
    with pytest.raises(UnsupportedModel, match="noise_shape"):
        _plan(desc)
    rc, _, err = _create_json(desc)
    assert rc == -2 and "noise_shape" in err   # IGN_ERR_UNSUPPORTED


def test_dropout_in_a_message_network_is_unsupported():
    desc = model_examples.routenet_message_net(units=(24, 32), iterations=3)
    for net in desc["neural_networks"]:
        if net["nn_name"] == "message_nn":
            net["nn_architecture"].insert(1, {"type_layer": "Dropout", "rate": 0.5})
    with pytest.raises(UnsupportedModel, match="message-creation network") as e:
        _plan(desc)
    rc, _, err = _create_json(desc)
    assert rc == -2 and err == str(e.value)


def test_other_layer_types_stay_refused():
    desc = dc.dropout_model("selu", [])
    for net in desc["neural_networks"]:
        if net["nn_name"] == "readout_model":
            net["nn_architecture"].insert(1, {"type_layer": "BatchNormalization"})
    with pytest.raises(UnsupportedModel, match="BatchNormalization"):
        _plan(desc)
    assert _create_json(desc)[0] == -2


def test_add_dropout_arguments_and_order():
    """ign_plan_add_dropout on a plan from ign_plan_create: argument checks, and refused once
    ign_batch_create was called on the plan."""
    plan = _plan(dc.readout_op_model())
    desc, keep = plan.to_desc()
    h = C.c_void_p()
    _lib.check(_lib.lib.ign_plan_create(C.byref(desc), 0, C.byref(h)))
    try:
        add = _lib.lib.ign_plan_add_dropout
        assert add(h, -1, 1, 0.5, 0) == 0
        assert add(h, -1, 2, 0.5, 0) == 0       # after the last of predict's two layers
        assert add(h, -1, 3, 0.5, 0) == -1
        assert add(h, 0, 2, 0.25, 7) == 0
        assert add(h, 1, 0, 0.5, 0) == -1       # the pooling operation has no Dense stack
        assert add(h, 5, 0, 0.5, 0) == -1
        assert add(h, -1, 0, 1.0, 0) == -1
        assert add(h, -1, 0, -0.1, 0) == -1
        assert add(h, -1, 0, 0.0, 0) == 0       # rate 0: accepted, no site
        bd = _lib.BatchDesc()                    # an empty description: the call fails, and closes the site list
        b = C.c_void_p()
        assert _lib.lib.ign_batch_create(h, C.byref(bd), C.byref(b)) != 0
        assert add(h, -1, 1, 0.5, 0) == -1
        assert "batch" in _lib.lib.ign_last_error().decode()
    finally:
        _lib.lib.ign_plan_destroy(h)


def test_trainer_refuses_before_the_gpu():
    """A Dropout model with an optimizer that is not lowered is still refused by the learning options,
    before torch or the engine are touched."""
    from ignnition_amd.training import Trainer
    desc = dc.dropout_model("selu", [(1, 0.5, {})])
    desc["learning_options"]["optimizer"] = {"type": "Nadam"}
    with pytest.raises(UnsupportedModel, match="Nadam"):
        Trainer(Model_information(copy.deepcopy(desc), DIMS))


def test_debug_dump_lists_the_sites(tmp_path):
    from ignnition_amd import framework_operations as fo
    mi = Model_information(dc.dropout_model("selu", [(1, 0.5, {"seed": 3})]), DIMS)
    dump = fo.debug(mi, str(tmp_path))
    assert dump["dropout_sites"] == [{"site": 0, "stack": -1, "before_layer": 1, "rate": 0.5, "seed": 3}]
