"""Randomised parity sweep of ps_kf_search and ps_search_by_sim3 against the numpy second opinion (developer tool, run on the GPU box):
the batches of tests/sweep_cases.py - the three modes and Sim3, 1 .. 4097 searched features in a random order, 1 .. 2000 points, dense
windows that overflow the everyday candidate store beside plain scenes that must not change, the searched side through a frame handle
now and then - on ONE matcher handle.  Every output is an integer and must be identical.  usage: stress_kfsearch.py [seed [budget]]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from pointslot_amd._lib import poison_lds
import parity_checks
import sweep_cases
from pointslot_amd.frame import DeviceFrame
from pointslot_amd.matcher import ORBmatcher

seed = int(sys.argv[1]) if len(sys.argv) > 1 else sweep_cases.COMMITTED["kfsearch"][0]
budget = int(sys.argv[2]) if len(sys.argv) > 2 else sweep_cases.COMMITTED["kfsearch"][1]
mt = ORBmatcher(0.6, True)
bad = nprob = skipped = 0
for it, call in enumerate(sweep_cases.calls("kfsearch", seed, budget)):
    poison_lds(0xFFFFFFFF if it % 2 == 0 else 0x7FF00000)      # uninitialised-LDS reads become deterministic failures
    refs = sweep_cases.reference_of("kfsearch", seed, call)
    frames = []
    if call["kind"] == "sim3":
        got = mt.SearchBySim3(call["problems"])
    else:
        probs = []
        for pr, via in zip(call["problems"], call["from_frame"]):
            if via:
                t = pr["train"]
                frame = DeviceFrame(len(t["x"]) + 5)
                frame.publish(t, None, t["desc"], t["grid"])
                frames.append(frame)
                pr = dict(pr, train=dict(frame=frame, occupied=t["occupied"]))
            probs.append(pr)
        got = mt.KfSearch(probs)
    for pr, g, ref in zip(call["problems"], got, refs):
        nprob += 1
        if sweep_cases.level_violations(ref)[0]:    # a predicted level within 4 ulp of a boundary: two correct implementations may differ
            skipped += 1
            continue
        try:
            if call["kind"] == "sim3":
                what = "sim3 n1 %d n2 %d s12 %g" % (len(pr["kf1"]["x"]), len(pr["kf2"]["x"]), pr["s12"])
                parity_checks.check_sim3(g, ref)
            else:
                what = "mode %d features %d points %d th %g th_dist %s orientation %s dense %s" % (
                    pr["mode"], len(pr["train"]["x"]), len(pr["query"]["valid"]), pr["th"], pr.get("th_dist"), pr.get("check_orientation"), "dense" in pr)
                parity_checks.check_kf(g, ref, pr["mode"])
        except AssertionError as e:
            bad += 1
            print("MISMATCH kfsearch seed %d call %d (%d problems): %s: %s" % (seed, it, len(got), what, str(e)[:300]))
    for f in frames:
        f.close()
mt.close()
if skipped * 50 > nprob:
    bad += 1
    print("MISMATCH kfsearch seed %d: %d of %d problems hold a level within 4 ulp of a boundary, more than 2 %%" % (seed, skipped, nprob))
print("stress_kfsearch: seed %d, %d problems, %d skipped (input condition), %d mismatches" % (seed, nprob, skipped, bad))
sys.exit(1 if bad else 0)
