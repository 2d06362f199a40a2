"""pose_lm runs a problem on one or four waves (PS_POSE_WAVES forces the form of a handle, the launcher's rule picks it otherwise; the two-wave
form won no row of the sweep and is not built).
Every form is held to the contract tests/test_opt_gpu.py states against the CPU oracle - return values and outlier masks exact, pose
within POSE_TOL, chi2 per iteration within rtol 1e-9, trial counts identical outside converged iterations - on edge counts that straddle
the lane / wave / unroll boundaries of the forms; within one form nothing depends on how many problems share the launch."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib
from pointslot_amd import synth
from test_opt_gpu import POSE_TOL, _cfse3_frame, _mat, _pose_err

pytestmark = pytest.mark.gpu
FORMS = (1, 4)


def _with_waves(value, make):
    """make() with PS_POSE_WAVES = value in the environment (None: unset): the handle reads it when it is created"""
    old = os.environ.get("PS_POSE_WAVES")
    try:
        if value is None:
            os.environ.pop("PS_POSE_WAVES", None)
        else:
            os.environ["PS_POSE_WAVES"] = str(value)
        return make()
    finally:
        if old is None:
            os.environ.pop("PS_POSE_WAVES", None)
        else:
            os.environ["PS_POSE_WAVES"] = old


@pytest.fixture(scope="module")
def opts():
    """one optimizer handle per forced form, and one that follows the rule (key 0)"""
    from pointslot_amd.optimizer import Optimizer
    o = {w: _with_waves(w, Optimizer) for w in FORMS}
    o[0] = _with_waves(None, Optimizer)
    o[2] = _with_waves(2, Optimizer)          # not a form: the rule
    yield o
    for h in o.values():
        h.close()


def _pose_frames():
    # the compaction walks 64-slot rows, 4 and 8 per step; the trial pass takes 4 edges per step and thread (64 / 128 / 256 threads)
    frames = [synth.pose_problem(0x600 + n, n=n) for n in (14, 15, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1025)]
    frames[0]["tcw0"] = frames[0]["tcw_true"].astype(np.float32)         # < 15 correspondences: the pose comes back untouched
    frames += [synth.pose_problem(0x700 + n, n=n, mono_frac=0.5, valid_frac=0.7) for n in (64, 129, 257, 513, 1025)]   # compacted index != slot index
    frames.append(synth.pose_problem(79, n=200, outlier_frac=0.6))
    frames.append(synth.pose_problem(81, n=120))                          # all information zero: the first factorisation fails
    frames[-1]["inv_sigma2"] = np.zeros_like(frames[-1]["inv_sigma2"])
    frames.append(synth.pose_problem(80, n=700, noise=3.0))
    frames[-1]["outlier0"] = (np.arange(700) % 7 == 0).astype(np.uint8)
    frames.append(synth.pose_problem(0x51070003))                         # one full-size frame: 2000 edges
    return frames


@pytest.fixture(scope="module")
def pose_cases():
    frames = _pose_frames()
    return frames, [oracle_lib.pose_optimize(f, True) for f in frames]


def _check_pose_batch(opt, frames, refs):
    """the assertions of test_opt_gpu.test_pose_optimization_batch"""
    opt.enable_trace(True)
    res = opt.PoseOptimization(frames)
    noise_only = []
    for i, (f, (r, tcw, outl)) in enumerate(zip(frames, res)):
        ro, to, oo, tro = refs[i]
        assert r == ro, (i, r, ro)
        assert np.array_equal(outl, oo), "frame %d: outlier masks differ at %d edges" % (i, (outl != oo).sum())
        assert _pose_err(tcw, to) <= POSE_TOL, (i, _pose_err(tcw, to))
        trg = opt.get_trace(i)
        if len(trg) != len(tro):
            # a converged iteration one side runs and the other does not (see test_pose_optimization_batch): it must leave chi2 where it was
            longer, shorter = (trg, tro) if len(trg) > len(tro) else (tro, trg)
            assert len(longer) - len(shorter) <= 2, (i, len(trg), len(tro))
            for r in longer:
                assert (np.abs(shorter[:, 0] - r[0]) <= 1e-10 * r[0]).any(), (i, r)
            noise_only.append(i)
            continue
        if len(tro):
            prev = np.concatenate([[np.inf], tro[:-1, 0]])
            converged = np.abs(prev - tro[:, 0]) <= 1e-10 * tro[:, 0]
            differ = trg[:, 2] != tro[:, 2]
            assert not (differ & ~converged).any(), (i, trg[:, 2], tro[:, 2])
            if differ.any():
                noise_only.append(i)
            assert np.allclose(trg[:, 0], tro[:, 0], rtol=1e-9)        # chi2 per iteration
            sig = (np.abs(prev - tro[:, 0]) > 1e-4 * tro[:, 0]) & (tro[:, 2] == 1)
            bad = ~np.isclose(trg[:, 1], tro[:, 1], rtol=1e-5) & sig
            assert not bad.any(), (i, trg[bad], tro[bad])
    assert np.array_equal(res[0][1], frames[0]["tcw0"])                # early return leaves the pose alone
    assert len(noise_only) <= len(frames) // 4, noise_only
    opt.enable_trace(False)


@pytest.mark.parametrize("nw", FORMS)
def test_pose_optimization_every_form(opts, pose_cases, nw):
    frames, refs = pose_cases
    _check_pose_batch(opts[nw], frames, refs)


def _cfse3_frames():
    frames = [_cfse3_frame(10 + k, k) for k in (1, 2, 3, 5, 16)]         # G side-by-side groups of the wide form / sequential vertices of the narrow one; 16 = PS_PO_MAX_K
    frames.append(_cfse3_frame(30, 1, npts=10))                          # fewer than 15 edges in total
    frames.append({"objs": [], "K": synth.pose_problem(1, 20)["K"]})     # no objects
    f = _cfse3_frame(31, 3)
    f["objs"][1]["valid"] = np.zeros_like(f["objs"][1]["valid"])          # one object without a valid edge beside two that have some
    frames.append(f)
    return frames


@pytest.fixture(scope="module")
def cfse3_cases():
    frames = _cfse3_frames()
    return frames, [oracle_lib.cfse3_optimize(f["objs"], f["K"]) for f in frames]


@pytest.mark.parametrize("nw", FORMS)
def test_cfse3_every_form(opts, cfse3_cases, nw):
    """the assertions of test_opt_gpu.test_cfse3_batch"""
    frames, refs = cfse3_cases
    res = opts[nw].CFSE3ObjStateOptimization(frames)
    for i, (f, (ok, poses, outls)) in enumerate(zip(frames, res)):
        oko, po, oo = refs[i]
        assert ok == oko, i
        for j in range(len(f["objs"])):
            assert np.array_equal(outls[j], oo[j]), (i, j)
            assert _pose_err(_mat(poses[j]), _mat(po[j])) <= POSE_TOL, (i, j)


def _same(a, b):
    return all(ra == rb and np.array_equal(ta.view(np.uint32), tb.view(np.uint32)) and np.array_equal(oa, ob) for (ra, ta, oa), (rb, tb, ob) in zip(a, b))


def test_form_identity(opts):
    import torch
    from pointslot_amd._lib import lib
    # a few problems: the path that did not change
    five = [synth.pose_problem(0x900 + k, n=300 + 100 * k) for k in range(5)]
    assert _same(opts[0].PoseOptimization(five), opts[4].PoseOptimization(five))
    assert _same(opts[0].PoseOptimization(five), opts[2].PoseOptimization(five))
    # one small problem per CU: the unforced handle runs the form the rule names
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(5)
    many = [synth.pose_problem(0xA00 + k, n=int(rng.integers(40, 121))) for k in range(cus)]
    lib.psk_pose_lm_waves.argtypes = [ctypes.c_int, ctypes.c_int]
    picked = lib.psk_pose_lm_waves(cus, 0)
    assert picked in FORMS
    assert lib.psk_pose_lm_waves(5, 0) == 4 and lib.psk_pose_lm_waves(5, 1) == 4
    unforced = opts[0].PoseOptimization(many)
    assert _same(unforced, opts[picked].PoseOptimization(many))
    # within one form nothing depends on who shares the launch
    for nw in FORMS:
        batch = unforced if nw == picked else opts[nw].PoseOptimization(many)
        alone = opts[nw].PoseOptimization([many[0]])
        last = opts[nw].PoseOptimization(many[1:] + [many[0]])
        assert _same(alone, batch[:1]), nw
        assert _same(alone, last[-1:]), nw
    # a launch the rule hands to the one-wave form (twice the batch: from two problems per CU on) equals the forced one-wave handle
    n1 = next(n for n in range(1, 64 * cus) if lib.psk_pose_lm_waves(n, 0) == 1)
    assert n1 <= 2 * len(many)
    twice = (many + many)[:n1]
    assert _same(opts[0].PoseOptimization(twice), opts[1].PoseOptimization(twice))


def test_tracker_one_wave_against_four():
    """LockstepTracker as in test_track_device_gpu.test_device_tracker_images_in_hbm_and_reset, once per form: the same frame records,
    poses within the file's device-versus-checker tolerance, and the one-wave form repeats itself bit for bit after reset()."""
    from pointslot_amd import sequence
    from pointslot_amd.tracker_device import LockstepTracker
    S, n = 3, 6
    seqs = [sequence.generate(n_frames=n, seed=80 + k, step=0.05 + 0.02 * k) for k in range(S)]
    h, w = seqs[0]["left"][0].shape

    def run(trk):
        for i in range(n):
            trk.step([np.ascontiguousarray(q["left"][i]) for q in seqs], [np.ascontiguousarray(q["right"][i]) for q in seqs])
        return trk.fetch()

    out = {}
    for nw in (1, 4):
        trk = _with_waves(nw, lambda: LockstepTracker(S, seqs[0]["K"], seqs[0]["bf"], w, h, max_steps=n))
        out[nw] = run(trk)
        if nw == 1:
            trk.reset()
            tcw_b, st_b = run(trk)
            assert np.array_equal(out[1][0].view(np.uint32), tcw_b.view(np.uint32))
            assert np.array_equal(out[1][1].view(np.int32), st_b.view(np.int32))
        trk.close()
    assert out[1][1]["tracked"].all()
    assert np.array_equal(out[1][1].view(np.int32), out[4][1].view(np.int32))
    assert np.abs(out[1][0].astype(np.float64) - out[4][0].astype(np.float64)).max() <= 2e-5
