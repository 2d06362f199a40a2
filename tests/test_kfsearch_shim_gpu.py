"""The loop-closure and relocalisation members of the C++ host shim (pointslot_amd/host/ORBmatcher.h) - SearchByProjection(pKF, Scw, ..),
Fuse(pKF, Scw, ..), SearchByProjection(CurrentFrame, pKF, ..) and SearchBySim3 - instantiated on the view types of tests/cpp/loop_view.h:
the pointers the reference-signature templates leave are those of the struct-level calls (tests/cpp/kfsearch_shim_check.cpp)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kfsearch_shim_check.cpp")


def _build(out):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pointslot_amd", "host"), "-I", os.path.join(ROOT, "include"),
                           SRC, "-o", out, "-L", os.path.join(ROOT, "pointslot_amd"), "-lpointslot_hip", "-pthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "pointslot_amd"), "-Wl,-rpath-link,/opt/rocm/lib"])
    return out


def test_kfsearch_shim_compiles_with_plain_gxx(tmp_path):
    exe = _build(str(tmp_path / "kfsearch_shim_check"))
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_kfsearch_shim_equals_the_struct_level_calls(tmp_path):
    exe = _build(str(tmp_path / "kfsearch_shim_check"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    summary = json.loads(lines[-1])
    assert summary["failed"] == 0 and summary["checks"] == 7, out.stdout
