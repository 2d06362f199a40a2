"""The drive generator's ray caster exists twice: the numpy statement (sequence._render_numpy) and the same per-pixel arithmetic as host C++
(pointslot_amd/csrc/seq_render.cpp -> libps_seqrender.so, what generate_drive uses when it is built).  They must agree bit for bit - float
image, depth and object ids - or tests and benchmark would see other images than before.  Small images, odd sizes, yaw of both signs, objects
in front of each other, a camera beside the corridor's middle."""
import numpy as np
import pytest

from pointslot_amd import sequence as S
from pointslot_amd.synth import KITTI_K


@pytest.fixture(scope="module")
def lib():
    lib = S._native_lib()
    assert lib, "libps_seqrender.so is missing: make -C pointslot_amd/csrc"
    return lib


@pytest.mark.parametrize("w,h,yaw,n_obj", [(1242, 375, 0.0, 2), (333, 117, 0.35, 0), (640, 201, -0.5, 5), (97, 61, 0.02, 1)])
def test_native_render_equals_the_numpy_statement_bit_for_bit(lib, w, h, yaw, n_obj):
    rng = np.random.default_rng(w + n_obj)
    mips = S._mip_chain(S.kitti_texture())
    fx, fy, cx, cy = [float(v) for v in KITTI_K]
    K = (fx * w / 1242.0, fy * w / 1242.0, (w - 1) / 2.0 + 0.25, (h - 1) / 2.0 - 0.5)
    cam = np.array([rng.uniform(-4, 4), rng.uniform(-0.3, 0.3), rng.uniform(0, 350)])
    objs = [(rng.uniform(-2, 2), 1.65, cam[2] + 6.0 + 3.0 * k, rng.uniform(1.6, 2.2), rng.uniform(1.3, 1.7), S._mip_chain(rng.uniform(0, 255, (80 + k, 110 + k)), 3))
            for k in range(n_obj)]
    a = S._render_numpy(cam, yaw, K, w, h, mips, objs)
    b = S._render_native(lib, cam, yaw, K, w, h, mips, objs, 40.0)
    assert b is not None
    for name, x, y in zip(("image", "depth", "object id"), a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    assert n_obj == 0 or (a[2] >= 0).any()


def test_generate_drive_is_the_same_sequence_with_either_renderer(lib, monkeypatch):
    kw = dict(n_frames=3, seed=47, speed=0.69, yaw_rate_deg=0.65, texture=S.kitti_texture(), n_objects=6, w=414, h=125)
    fast = S.generate_drive(**kw)
    monkeypatch.setattr(S, "_render", S._render_numpy)
    slow = S.generate_drive(**kw)
    for k in ("left", "right", "seg", "twc"):
        assert np.array_equal(fast[k], slow[k]), k
    assert fast["boxes"] == slow["boxes"] and fast["labels"] == slow["labels"]
