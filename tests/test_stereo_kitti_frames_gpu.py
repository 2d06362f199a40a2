"""examples/stereo_kitti with PS_ODO_DEVICE_FRAMES=1: the single-sequence driver publishes every frame once into a frame handle
after ComputeStereoMatches and serves its 2-3 searches from it - to the byte the trajectory of the default (host-array) path."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_stereo_kitti_with_frame_handles_writes_the_same_trajectory(tmp_path):
    from pointslot_amd import sequence
    exe = str(tmp_path / "stereo_kitti")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "pointslot_amd", "host"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "stereo_kitti.cpp"), "-o", exe, "-L", os.path.join(ROOT, "pointslot_amd"),
                           "-lpointslot_hip", "-pthread", "-Wl,-rpath," + os.path.join(ROOT, "pointslot_amd"), "-Wl,-rpath-link,/opt/rocm/lib"])
    seq = sequence.generate(n_frames=8, seed=4)
    d = str(tmp_path / "0000")
    sequence.write(d, seq, pgm=True)
    got = {}
    for switch in ("0", "1"):
        env = dict(os.environ, PS_ODO_DEVICE_FRAMES=switch)
        if switch == "0":
            env.pop("PS_ODO_DEVICE_FRAMES")
        out = subprocess.run([exe, d], capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
        assert "trajectory saved!" in out.stdout and "LOST" not in out.stdout
        assert ("frame handles: on" in out.stdout) == (switch == "1")
        got[switch] = (open(os.path.join(d, "CameraTrajectory.txt"), "rb").read(), [l for l in out.stdout.splitlines() if l.startswith("frame ") and l[6:7].isdigit()])
    assert len(got["0"][0].splitlines()) == 8
    assert got["0"][0] == got["1"][0]
    assert got["0"][1] == got["1"][1]          # match counts per frame
