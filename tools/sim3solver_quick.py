"""Developer tool: the loop-closure Sim3 solver at the workload's shape (scenes drawn as in tests/sim3solver_cases.py).
  ps_sim3_ransac   LoopClosing::ComputeSim3: 1 / 8 candidate keyframe pairs x 300 hypotheses at N = 150 and N = 1000 correspondences,
                   half of them wrong, one batched call with the masks read back
Per shape: the kernel time (ps_matcher_last_kernel_ms) and the wall time of the call - median of 20 calls after 3 warm-up calls,
with the least and the greatest.  There is no CPU baseline for this call: the figures are the GPU's alone.
--json PATH writes the figures as JSON (default profiles/sim3solver_quick.json)."""
import json, os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import sim3solver_cases as sc
from pointslot_amd.matcher import ORBmatcher
from pointslot_amd.sim3solver import sim3_ransac

WARM, REPS, NHYP = 3, 20, 300


def stats(x):
    return dict(median=float(np.median(x)), least=float(np.min(x)), greatest=float(np.max(x)))


def timed(matcher, call):
    ker, wall = [], []
    for it in range(WARM + REPS):
        t0 = time.perf_counter()
        res = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ker.append(matcher.last_kernel_ms())
    return dict(kernel_ms=stats(ker[WARM:]), call_ms=stats(wall[WARM:])), res


matcher = ORBmatcher(0.6, True)
out = {"hypotheses_per_candidate": NHYP, "warmup": WARM, "repeats": REPS, "cpu_baseline": "none: GPU figures only"}
for n in (150, 1000):
    probs = [sc.problem(sc.scene(800 + k, n, 0.5, 0.5, k % 2 == 1, min_inliers=20, nhyp=NHYP)) for k in range(8)]
    for count in (1, 8):
        r, res = timed(matcher, lambda: sim3_ransac(matcher, probs[:count]))
        r["first_success"] = [int(x["first_success"]) for x in res]
        r["most_inliers"] = [int(x["inliers"].max()) for x in res]
        out["ransac_%d_candidates_n%d" % (count, n)] = r
        print("ps_sim3_ransac: %d candidates x %d hypotheses, N = %d: kernel %.3f ms, call %.3f ms, first success at %s"
              % (count, NHYP, n, r["kernel_ms"]["median"], r["call_ms"]["median"], r["first_success"]), flush=True)
matcher.close()
path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv[1:] else os.path.join(ROOT, "profiles", "sim3solver_quick.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
