"""Randomised parity sweeps as part of the GPU suite: the developer tools under tools/stress_*.py - random image sizes, strides, pyramid
parameters, masks, matcher scenes and optimiser graphs against the CPU checker, bit for bit - run here with a fixed seed and a small
budget each (a few seconds), so that every GPU test run also covers shapes no hand-written case has (tile / cell / tap edge cases of the
extraction kernels in particular).  The tools exit non-zero on the first difference.  The sweeps of the mapping and place-recognition
calls (tests/sweep_cases.py; tests/test_sweep_cases_cpu.py checks their input conditions and what they reach under these very seeds)
run a second time with every fresh device buffer filled with 0xFF bytes: their scratch comes from the matcher's arena.  So does the
sweep of the stereo matcher (tests/stereo_cases.py, tests/test_stereo_cases_cpu.py): its result, SAD and row-bucket buffers and the
key sets' staging buffer are poisoned with the pyramid arena.  The committed scenes of the tracking thread's matchers
(tests/match_cases.py, tests/test_match_cases_cpu.py; tools/stress_matchers.py --cases) run both ways as well: candidate keys, claim
tables' backing store and the published frames all come from fresh device buffers."""
import os
import subprocess
import sys

import pytest

import sweep_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _committed(family):
    return [str(v) for v in sweep_cases.COMMITTED[family]]


SWEEPS = [
    ("stress_orb.py", ["20250501", "60"], "0 mismatches"),                    # ORBextractor: 60 random images / parameter sets
    ("stress_cvorb_batch.py", ["20250502", "12"], "identical to the CPU restatement"),   # batched cv::ORB stand-in under random masks
    ("stress_matchers.py", ["20250503"], "0 mismatches"),                     # the matchers' scenes
    ("stress_opt.py", ["20250504"], "0 mismatches"),                          # PoseOptimization / CFSE3 / object BA graphs
    ("stress_tri.py", _committed("tri"), "0 mismatches"),                     # CreateNewMapPoints: search, triangulation, chain
    ("stress_bow.py", _committed("bow"), "0 mismatches"),                     # ComputeBoW and SearchByBoW in turn on one handle
    ("stress_kfdb.py", _committed("kfdb"), "0 mismatches"),                   # KeyFrameDatabase scripts: add / erase / clear / query / score
    ("stress_kfsearch.py", _committed("kfsearch"), "0 mismatches"),           # loop-closure / relocalisation projections and SearchBySim3
    ("stress_stereo.py", _committed("stereo"), "0 mismatches"),               # ComputeStereoMatches (two handles, batch) and ComputeObjStereoMatches
    ("stress_matchers.py", ["--cases"] + _committed("match"), "0 mismatches"),   # the matchers' committed scenes, from host arrays and from frames
]
# the second run, on poisoned device memory: every sweep of committed scenes (tri, bow, kfdb, kfsearch, stereo and the matchers' cases)
POISONED = SWEEPS[4:]
assert [s[0] for s in POISONED] == ["stress_tri.py", "stress_bow.py", "stress_kfdb.py", "stress_kfsearch.py", "stress_stereo.py", "stress_matchers.py"]


def _ids(sweeps):
    return [s[0][:-3] + ("_cases" if s[1][:1] == ["--cases"] else "") for s in sweeps]


def _sweep(tool, args, expect, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)] + args, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert expect in r.stdout, tail


@pytest.mark.gpu
@pytest.mark.parametrize("tool,args,expect", SWEEPS, ids=_ids(SWEEPS))
def test_random_sweep(tool, args, expect):
    _sweep(tool, args, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("tool,args,expect", POISONED, ids=_ids(POISONED))
def test_random_sweep_with_poisoned_device_memory(tool, args, expect):
    _sweep(tool, args, expect, dict(os.environ, PS_DEBUG_FILL="255"))
