"""The training-table lowering (ignnition_amd/csrc/train_lower.cpp) on the CPU: tests/cpp/train_lower_check.cpp
holds the smallest cases with their transposed CSRs written out by hand, the host tables they read
produced by the batch lowering where it accepts the case.  It is built with g++ as a stand-alone
program -- no HIP, no Python extension -- and run plain and under the address / undefined-behaviour
sanitizers."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "train_lower_check.cpp"),
           os.path.join(ROOT, "ignnition_amd", "csrc", "train_lower.cpp"),
           os.path.join(ROOT, "ignnition_amd", "csrc", "batch_lower.cpp")]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_train_lower_check(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the lowering check"
    exe = str(tmp_path / "train_lower_check")
    cc = subprocess.run([gxx, "-std=c++17", "-Wall", *flags, *SOURCES, "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
