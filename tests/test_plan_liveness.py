"""Which MPs' last-iteration update nothing reads (MPP::dead_in_last_iter, plan_lower.cpp), on the CPU.
tests/cpp/plan_liveness_check.cpp lowers small hand-written plans through the HIP-free unit, built with
g++ as a stand-alone program and run plain and under the address / undefined-behaviour sanitizers; the
example models' own descriptions are lowered through the library (no device is touched) and read back
with ign_plan_mp_dead_last, as the debug dump shows them."""

import copy
import os
import shutil
import subprocess

import pytest

from ignnition_amd import framework_operations as fo
from ignnition_amd import model_examples, workloads
from ignnition_amd.engine import MPPlan
from ignnition_amd.json_operations import Model_information

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "plan_liveness_check.cpp"),
           os.path.join(ROOT, "ignnition_amd", "csrc", "plan_lower.cpp")]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_plan_liveness_check(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the lowering check"
    exe = str(tmp_path / "plan_liveness_check")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", *flags, *SOURCES, "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]


def _flags(mi):
    plan = MPPlan.from_model_info(mi)
    return {plan.entities[m["dst"]]: d for m, d in zip(plan.mps, plan.dead_in_last_iter())}, plan


def test_routenet_link_update_is_dead():
    flags, plan = _flags(workloads.model("routenet")[2])
    assert [plan.entities[m["dst"]] for m in plan.mps] == ["path", "link"]
    assert flags == {"path": False, "link": True}


def test_qsize_link_and_node_updates_are_dead():
    flags, _ = _flags(workloads.model("qsize")[2])
    assert flags == {"path": False, "link": True, "node": True}


def test_single_entity_model_has_no_dead_update():
    flags, _ = _flags(workloads.make_synthetic_inputs(n_nodes=50, iterations=2, window=8)[2])
    assert flags == {"node": False}


def test_routenet_predicting_on_links_has_no_dead_update():
    desc = model_examples.routenet()
    desc["readout"][0]["input"] = ["link"]
    _, dims, _ = workloads.model("routenet")
    flags, _ = _flags(Model_information(copy.deepcopy(desc), dims))
    assert flags == {"path": False, "link": False}


def test_switch_leaves_the_flag(monkeypatch):
    """IGN_DEAD_LAST=0 keeps ign_forward from using the flag; the flag itself is the model's."""
    monkeypatch.setenv("IGN_DEAD_LAST", "0")
    flags, _ = _flags(workloads.model("routenet")[2])
    assert flags == {"path": False, "link": True}


def test_debug_dump_lists_the_flags(tmp_path):
    dump = fo.debug(workloads.model("qsize")[2], str(tmp_path))
    assert dump["dead_in_last_iter"] == [False, True, True]
    assert len(dump["dead_in_last_iter"]) == len(dump["message_passings"])
