"""Randomised parity sweep of ps_bow_transform and ps_search_by_bow against the second opinion (developer tool, run on the GPU box):
the calls of tests/sweep_cases.py - trees of k = 2 .. 20 and L = 2 .. 6 with pruning, stopped words and tied siblings, the four
weightings, frames of 0 .. 2000 features with many distinct words or with runs of hundreds of equal ones, and searches over sides of
1 .. 2000 features - transform and search in turn on ONE matcher handle.  usage: stress_bow.py [seed [budget]]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from pointslot_amd._lib import poison_lds
import parity_checks
import sweep_cases
from pointslot_amd import bow
from pointslot_amd.matcher import ORBmatcher

seed = int(sys.argv[1]) if len(sys.argv) > 1 else sweep_cases.COMMITTED["bow"][0]
budget = int(sys.argv[2]) if len(sys.argv) > 2 else sweep_cases.COMMITTED["bow"][1]
mt = ORBmatcher(0.6, True)
vocs = {}
bad = nprob = 0
for it, call in enumerate(sweep_cases.calls("bow", seed, budget)):
    poison_lds(0xFFFFFFFF if it % 2 == 0 else 0x7FF00000)      # uninitialised-LDS reads become deterministic failures
    refs = sweep_cases.reference_of("bow", seed, call)
    if call["kind"] == "transform":
        tree = call["tree"]
        if tree not in vocs:
            vocs[tree] = bow.Vocabulary.from_arrays(**sweep_cases.bow_vocabulary(seed, *tree))
        got = vocs[tree].transform(call["frames"], call["levelsup"], matcher=mt)
        for f, lv, mix, g, ref in zip(call["frames"], call["levelsup"], call["mixes"], got, refs):
            nprob += 1
            try:
                parity_checks.check_transform(g, ref, len(f))
            except AssertionError as e:
                bad += 1
                print("MISMATCH bow transform seed %d call %d (%d frames): tree k %d L %d n %d levelsup %d bases %d: %s" %
                      (seed, it, len(got), tree[0], tree[1], len(f), lv, mix, str(e)[:300]))
    else:
        got = mt.SearchByBoWBatch(call["problems"])
        for pr, g, ref in zip(call["problems"], got, refs):
            nprob += 1
            try:
                parity_checks.check_bow_search(g, ref)
            except AssertionError as e:
                bad += 1
                print("MISMATCH bow search seed %d call %d (%d problems): na %d nb %d mode %d nn_ratio %g orientation %d: %s" %
                      (seed, it, len(got), len(pr["a"]["node"]), len(pr["b"]["node"]), pr["mode"], pr["nn_ratio"], pr["check_orientation"], str(e)[:300]))
for v in vocs.values():
    v.close()
mt.close()
print("stress_bow: seed %d, %d frames and searches, %d mismatches" % (seed, nprob, bad))
sys.exit(1 if bad else 0)
