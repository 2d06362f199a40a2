"""Randomised parity sweep of ps_create_new_map_points against the numpy second opinion (developer tool, run on the GPU box): the
batches of tests/sweep_cases.py - n1 and n2 around a wave, a workgroup and several of them, 1 .. 32 neighbours, node lists shorter and
longer than a wave, every setting drawn at random, keyframe 1 through a frame handle now and then - on ONE matcher handle, so the
arena grows, shrinks and is reused with stale contents.  usage: stress_tri.py [seed [budget]]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
from pointslot_amd._lib import poison_lds
import parity_checks
import sweep_cases
from pointslot_amd.frame import DeviceFrame
from pointslot_amd.matcher import ORBmatcher

seed = int(sys.argv[1]) if len(sys.argv) > 1 else sweep_cases.COMMITTED["tri"][0]
budget = int(sys.argv[2]) if len(sys.argv) > 2 else sweep_cases.COMMITTED["tri"][1]
GRID = (0.0, 0.0, np.float32(64) / np.float32(1241), np.float32(48) / np.float32(376))
HELD = ("depth", "node", "occupied", "x_raw", "y_raw", "R", "t", "ow", "K8", "scale_factors", "level_sigma2")
mt = ORBmatcher(0.6, False)
bad = nprob = skipped = 0
for it, call in enumerate(sweep_cases.calls("tri", seed, budget)):
    poison_lds(0xFFFFFFFF if it % 2 == 0 else 0x7FF00000)      # uninitialised-LDS reads become deterministic failures
    refs = sweep_cases.reference_of("tri", seed, call)
    probs, frames = [], []
    for pr, via in zip(call["problems"], call["from_frame"]):
        if via:
            kf1 = pr["kf1"]
            frame = DeviceFrame(len(kf1["node"]) + 7)
            frame.publish(kf1, kf1["u_right"], kf1["desc"], GRID)
            frames.append(frame)
            pr = dict(pr, kf1=dict({k: kf1[k] for k in HELD if k in kf1}, frame=frame))
        probs.append(pr)
    got = mt.CreateNewMapPoints(probs)
    for pr, g, ref in zip(call["problems"], got, refs):
        nprob += 1
        if sweep_cases.tri_bad_pairs(ref):          # an unstable or ill-conditioned pair: two correct implementations may differ
            skipped += 1
            continue
        try:
            parity_checks.check_tri(g, ref)
        except AssertionError as e:
            bad += 1
            s = pr["settings"]
            print("MISMATCH tri seed %d call %d (%d problems): n1 %d n2 %s settings %s: %s" %
                  (seed, it, len(probs), s["n1"], s["n2"], {k: v for k, v in s.items() if k not in ("n1", "n2")}, str(e)[:300]))
    for f in frames:
        f.close()
mt.close()
if skipped * 50 > nprob:
    bad += 1
    print("MISMATCH tri seed %d: %d of %d problems hold an unstable or ill-conditioned pair, more than 2 %%" % (seed, skipped, nprob))
print("stress_tri: seed %d, %d problems, %d skipped (input condition), %d mismatches" % (seed, nprob, skipped, bad))
sys.exit(1 if bad else 0)
