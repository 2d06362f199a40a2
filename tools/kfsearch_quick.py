"""Developer tool: the loop-closure and relocalisation projection matchers at the workload's shape (scenes drawn as in
tests/kfsearch_cases.py: 1241 x 376, 8 levels, 1500 features per keyframe).
  Fuse(pKF, Scw, ..)          LoopClosing::SearchAndFuse: 1 / 8 / 32 connected keyframes x 2000 loop map points, one batched call
  SearchBySim3                LoopClosing::ComputeSim3: 1 / 8 candidate keyframes, 1500 slots a side, one batched call
  SearchByProjection(F, pKF)  Tracking::Relocalization: 1 / 8 candidate keyframes of 1500 slots against ONE frame, from host arrays
                              and from a frame handle published once
Per shape: the kernel time (ps_matcher_last_kernel_ms) and the wall time of the call - median of 20 calls after 3 warm-up calls,
with the least and the greatest.  --json PATH writes the figures as JSON (default profiles/kfsearch_quick.json)."""
import json, os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import kfsearch_cases as kc
from pointslot_amd.frame import DeviceFrame
from pointslot_amd.matcher import ORBmatcher

WARM, REPS, NF = 3, 20, 1500


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
out = {"features_per_keyframe": NF, "warmup": WARM, "repeats": REPS}
fuse = [kc._main(1, 500 + k, nf=NF, nq=2000, th=4.0) for k in range(32)]
for count in (1, 8, 32):
    r, res = timed(matcher, lambda: matcher.FuseSim3(fuse[:count]))
    r["fused"] = int(sum((bi >= 0).sum() for bi, _ in res))
    out["fuse_%d_keyframes_x_2000_points" % count] = r
    print("Fuse(pKF, Scw): %2d keyframes x 2000 points: kernels %.3f ms, call %.3f ms, %d fused" % (count, r["kernel_ms"]["median"], r["call_ms"]["median"], r["fused"]), flush=True)
sim3 = [kc._sim3(600 + k, (1.0, 0.93)[k % 2], n=NF) for k in range(8)]
for count in (1, 8):
    r, res = timed(matcher, lambda: matcher.SearchBySim3(sim3[:count]))
    r["found"] = int(sum(x["nfound"] for x in res))
    out["sim3_%d_candidates" % count] = r
    print("SearchBySim3: %d candidates: kernels %.3f ms, call %.3f ms, %d found" % (count, r["kernel_ms"]["median"], r["call_ms"]["median"], r["found"]), flush=True)
base = kc._main(2, 700, nf=NF, nq=NF, th=10.0, th_dist=100)
rng = np.random.RandomState(7)
cands = [dict(base, query=dict(base["query"], valid=(base["query"]["valid"] * (rng.rand(NF) < 0.7)).astype(np.uint8))) for _ in range(8)]
frame = DeviceFrame(NF)
frame.publish(base["train"], None, base["train"]["desc"], base["train"]["grid"])
held = [dict(p, train=dict(frame=frame, occupied=p["train"]["occupied"])) for p in cands]
for count in (1, 8):
    for name, probs in (("host_arrays", cands), ("frame_handle", held)):
        r, res = timed(matcher, lambda: matcher.SearchByProjectionKeyFrame(probs[:count]))
        r["matches"] = int(sum(n for n, _ in res))
        out["relocalisation_%d_candidates_%s" % (count, name)] = r
        print("SearchByProjection(F, pKF): %d candidates, %s: kernels %.3f ms, call %.3f ms, %d matches" % (count, name, r["kernel_ms"]["median"], r["call_ms"]["median"], r["matches"]), flush=True)
frame.close()
matcher.close()
path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv[1:] else os.path.join(ROOT, "profiles", "kfsearch_quick.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
