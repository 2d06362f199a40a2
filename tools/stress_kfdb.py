"""Randomised parity sweep of the keyframe database (ps_kfdb_*) against the second opinion (developer tool, run on the GPU box): the
scripts of tests/sweep_cases.py - adds, erases, re-adds, a clear, queries in calls of 1 .. 8 in mixed modes and scores over stored
vectors of 0 .. 2000 words, and about 2100 short vectors asked with 4 and 6 queries - played on databases that share ONE matcher
handle.  Everything is equal, not close: lists, counts, float and double bits.  usage: stress_kfdb.py [seed [budget]]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from pointslot_amd._lib import poison_lds
import parity_checks
import sweep_cases
from pointslot_amd import kfdb
from pointslot_amd.matcher import ORBmatcher

seed = int(sys.argv[1]) if len(sys.argv) > 1 else sweep_cases.COMMITTED["kfdb"][0]
budget = int(sys.argv[2]) if len(sys.argv) > 2 else sweep_cases.COMMITTED["kfdb"][1]
mt = ORBmatcher(0.6, True)
bad = nres = 0
for it, case in enumerate(sweep_cases.calls("kfdb", seed, budget)):
    poison_lds(0xFFFFFFFF if it % 2 == 0 else 0x7FF00000)      # uninitialised-LDS reads become deterministic failures
    refs = sweep_cases.reference_of("kfdb", seed, case)
    db = kfdb.KeyFrameDatabase(case["capacity"], case["max_words"], matcher=mt)
    got = parity_checks.play_kfdb_device(db, case)
    db.close()
    if len(got) != len(refs):
        bad += 1
        print("MISMATCH kfdb seed %d case %s: %d results, the second opinion has %d" % (seed, case["name"], len(got), len(refs)))
    for k, (g, ref) in enumerate(zip(got, refs)):
        nres += 1
        try:
            if "scores" in ref:
                parity_checks.check_kfdb_score(g["scores"], ref["scores"])
            else:
                parity_checks.check_kfdb_query(g, ref)
        except AssertionError as e:
            bad += 1
            q = ref.get("query")
            what = "score over %d keyframes" % len(ref["scores"]) if q is None else "query %d mode %d words %d excluded %d shares %d" % (
                q["qid"], q["mode"], len(q["bow"][0]), len(q["connected"]), len(ref["share_id"]))
            print("MISMATCH kfdb seed %d case %s (capacity %d, max_words %d) result %d: %s: %s" %
                  (seed, case["name"], case["capacity"], case["max_words"], k, what, str(e)[:300]))
mt.close()
print("stress_kfdb: seed %d, %d query and score results, %d mismatches" % (seed, nres, bad))
sys.exit(1 if bad else 0)
