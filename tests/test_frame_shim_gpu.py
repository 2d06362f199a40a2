"""The frame-handle binding of the C++ host shims (pointslot_amd/host/ORBmatcher.h): a Frame type with a `ps_frame* mpDeviceFrame`
member searches through the handle when it is set; return values and written pointers are those of the host-array path
(tests/cpp/frame_handle_check.cpp)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "frame_handle_check.cpp")


def _build(out):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pointslot_amd", "host"), "-I", os.path.join(ROOT, "include"),
                           SRC, "-o", out, "-L", os.path.join(ROOT, "pointslot_amd"), "-lpointslot_hip", "-pthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "pointslot_amd"), "-Wl,-rpath-link,/opt/rocm/lib"])
    return out


def test_frame_handle_binding_compiles_with_plain_gxx(tmp_path):
    exe = _build(str(tmp_path / "frame_handle_check"))
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_frame_handle_binding_equals_the_host_array_path(tmp_path):
    exe = _build(str(tmp_path / "frame_handle_check"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    summary = json.loads(lines[-1])
    assert summary["failed"] == 0 and summary["checks"] == 4, out.stdout
    for name in ("SearchByProjection(CurrentFrame, LastFrame, th, bMono) with mpDeviceFrame", "SearchByProjection(F, vpMapPoints, th) with mpDeviceFrame",
                 "Fuse(pKF, vpMapPoints, th) search half through the handle"):
        assert any(l.startswith("ok") and name in l for l in lines), name
