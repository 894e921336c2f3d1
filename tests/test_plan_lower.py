"""The plan lowering (ignnition_amd/csrc/plan_lower.cpp) on the CPU: tests/cpp/plan_lower_check.cpp writes
five small plans out as ign_plan_descs and checks the parameter layout against tables worked out by hand,
the invariants that tie the packed layout to its pack list, every refusal's code and text, and the
training switches.  It is built with g++ as a stand-alone program -- no HIP, no Python extension -- and
run plain and under the address / undefined-behaviour sanitizers."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "plan_lower_check.cpp"),
           os.path.join(ROOT, "ignnition_amd", "csrc", "plan_lower.cpp")]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_plan_lower_check(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the lowering check"
    exe = str(tmp_path / "plan_lower_check")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", *flags, *SOURCES, "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
