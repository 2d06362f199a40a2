"""The C++ Sim3Solver of the host shim (pointslot_amd/host/Sim3Solver.h) instantiated on the view types of tests/cpp/loop_view.h: the
constructor's filters and mvnIndices1, the truncated gates, iterate(5) against a walk over the struct-level call, and PrepareBatch over
three solvers against three single runs (tests/cpp/sim3solver_shim_check.cpp)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim3solver_shim_check.cpp")


def _build(out):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pointslot_amd", "host"), "-I", os.path.join(ROOT, "include"),
                           SRC, "-o", out, "-L", os.path.join(ROOT, "pointslot_amd"), "-lpointslot_hip", "-pthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "pointslot_amd"), "-Wl,-rpath-link,/opt/rocm/lib"])
    return out


@pytest.mark.gpu
def test_sim3solver_shim_equals_the_struct_level_call(tmp_path):
    exe = _build(str(tmp_path / "sim3solver_shim_check"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    summary = json.loads(lines[-1])
    assert summary["failed"] == 0 and summary["checks"] == 7, out.stdout
