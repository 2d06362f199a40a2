"""KeyFrameDatabase of the C++ host shims (pointslot_amd/host/KeyFrameDatabase.h) instantiated on the KeyFrame- / Frame-shaped types
of tests/cpp/kfdb_view.h: what the reference-signature calls return is what the struct-level calls return on the same data
(tests/cpp/kfdb_shim_check.cpp)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kfdb_shim_check.cpp")


def _build(out):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pointslot_amd", "host"), "-I", os.path.join(ROOT, "include"),
                           SRC, "-o", out, "-L", os.path.join(ROOT, "pointslot_amd"), "-lpointslot_hip", "-pthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "pointslot_amd"), "-Wl,-rpath-link,/opt/rocm/lib"])
    return out


def test_kfdb_shim_compiles_with_plain_gxx(tmp_path):
    exe = _build(str(tmp_path / "kfdb_shim_check"))
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_kfdb_shim_equals_the_struct_level_calls(tmp_path):
    exe = _build(str(tmp_path / "kfdb_shim_check"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    summary = json.loads(lines[-1])
    assert summary["failed"] == 0 and summary["checks"] == 7, out.stdout
