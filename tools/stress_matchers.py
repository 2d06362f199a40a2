"""Parity sweeps of the order-dependent matchers against the CPU checker, bit for bit (developer tool, run on the GPU box).

  stress_matchers.py [seed [scenes]]              many random scene seeds and sizes, dense scenes with heavy competition for the same
                                                  keypoints included (random_scenes below; needs nothing of tests/match_cases.py
                                                  unless a call has to be skipped)
  stress_matchers.py --cases [seed [budget]]      the scenes of tests/match_cases.py, whose gates tests/test_match_cases_cpu.py counts:
                                                  every call from host arrays and, for the projection and Fuse problems, a second time
                                                  with the searched sides published as DeviceFrames, on ONE matcher handle, so that the
                                                  scratch of a larger earlier scene lies under a smaller later one

Only the documented capacity error ("more than 1024 candidates" in a search window) lets a call be skipped: never on the committed
scenes, and on the random ones only where the second opinion counts such a window.  Exit status 1 on any difference."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
from pointslot_amd._lib import poison_lds, PointslotError, PS_ERR_CAPACITY
import oracle_lib
from pointslot_amd import synth
from pointslot_amd.matcher import ORBmatcher, build_grid

bad = skipped = unpredicted = 0


def capacity(e):
    """the one error a sweep may meet: a window beyond the wide candidate store"""
    return isinstance(e, PointslotError) and e.code == PS_ERR_CAPACITY and "more than 1024 candidates" in str(e)


def mismatch(what, detail):
    global bad
    bad += 1
    print("MISMATCH %s: %s" % (what, detail))


def same(got, ref):
    """(nmatches, array) or (best_idx, best_dist) of the device against the reference's; None, or what differs"""
    if np.isscalar(ref[0]) or isinstance(ref[0], int):
        if got[0] != ref[0] or len(got[1]) != len(ref[1]) or not np.array_equal(got[1], ref[1]):
            return "%d vs %d matches, %s slots differ" % (got[0], ref[0], int((got[1] != ref[1]).sum()) if len(got[1]) == len(ref[1]) else "all")
        return None
    nd = [int((np.asarray(g) != np.asarray(r)).sum()) if len(g) == len(r) else -1 for g, r in zip(got, ref)]
    return None if nd == [0, 0] else "%d best_idx and %d best_dist values differ" % tuple(nd)


# ---- the random scenes -------------------------------------------------------------------------------------------------------------
def random_scenes(seed, nscenes):
    """the settings of the random scenes for `seed`, in the draw order this tool has always had (numpy's generator: the committed
    runs `20250503` and `11 16` keep their scenes)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nscenes):
        s = dict(n=int(rng.choice([60, 300, 1000, 2000, 3000])), m=int(rng.choice([40, 500, 1500, 4000])), th=float(rng.choice([3.0, 7.0, 15.0, 30.0])))
        s["w"], s["h"] = (1241, 376) if rng.random() < 0.7 else (400, 200)       # the small image makes many queries fight for few keypoints
        s["seed"] = int(rng.integers(1, 1 << 30))
        s["th_points"] = float(rng.choice([1.0, 3.0]))
        s["ratios"] = {True: float(rng.choice([0.6, 0.8, 0.9])), False: float(rng.choice([0.6, 0.8, 0.9]))}       # by check_ori, in the order of the calls
        s["bf"] = dict(nq=int(rng.choice([10, 300, 1000])), nt=int(rng.choice([12, 320, 1000])), dup_frac=float(rng.choice([0.1, 0.5])))
        s["fuse_th"] = float(rng.choice([3.0, 5.0]))
        out.append(s)
    return out


def random_scene_problems(s):
    """-> (the three projection problems, the brute-force problem, the Fuse problem) of one random scene"""
    sc = synth.projection_scene(s["seed"], n=s["n"], m=s["m"], w=s["w"], h=s["h"], th=s["th"])
    tr = dict(sc["train"]); tr["cell_off"], tr["cell_idx"] = build_grid(tr["x"], tr["y"], *tr["grid"])
    common = {"train": tr, "scale_factors": sc["scale_factors"]}
    probs = [dict(common, mode="frame", query=sc["frame_query"], tcw=sc["tcw"], tlw=sc["tlw"], K6=sc["K6"], bounds=sc["bounds"], th=s["th"]),
             dict(common, mode="points", query=sc["points_query"], th=s["th_points"]),
             dict(common, mode="points", query=sc["points_query"], th=5.0, object=True)]
    bp = synth.bruteforce_problem(s["seed"], **s["bf"])
    fs = synth.fuse_scene(s["seed"], n=s["n"], m=min(s["m"], 2500), th=s["fuse_th"])
    T = fs["train"]; T["cell_off"], T["cell_idx"] = build_grid(T["x"], T["y"], *T["grid"])
    return probs, bp, fs


def run_random(seed, nscenes):
    global skipped, unpredicted
    for it, s in enumerate(random_scenes(seed, nscenes)):
        poison_lds(0xFFFFFFFF if it % 2 == 0 else 0x7FF00000)      # uninitialised-LDS reads become deterministic failures
        probs, bp, fs = random_scene_problems(s)
        for check_ori in (True, False):
            mt = ORBmatcher(s["ratios"][check_ori], check_ori)
            try:
                res = mt.SearchByProjection(probs)
            except PointslotError as e:      # candidate-list capacity on very dense scenes is a documented limit
                if not capacity(e):
                    raise
                skipped += 1
                import match_cases                  # (the counted second opinion: only a skipped call needs it)
                predicted = match_cases.windows_over_1024(probs, mt.mfNNratio)
                unpredicted += predicted == 0
                print("scene %d: %s (the second opinion counts %d windows over 1024)" % (it, str(e)[:80], predicted)); mt.close(); continue
            for pr, got in zip(probs, res):
                ref = oracle_lib.search_projection_frame(pr, check_ori) if pr["mode"] == "frame" else oracle_lib.search_projection_points(pr, mt.mfNNratio)
                msg = same(got, ref)
                if msg:
                    mismatch("scene %d seed %d n %d m %d th %g mode %s obj %s ori %s" % (it, s["seed"], s["n"], s["m"], s["th"], pr["mode"], pr.get("object"), check_ori), msg)
            mt.close()
        mt = ORBmatcher(0.9, True)
        (got,) = mt.SearchByBruceMatching([bp])
        if same(got, oracle_lib.search_bruteforce(bp, 0.9, True)):
            mismatch("bruteforce seed %d" % s["seed"], same(got, oracle_lib.search_bruteforce(bp, 0.9, True)))
        (got,) = mt.FuseSearch([fs])
        if same(got, oracle_lib.fuse_search(fs)):
            mismatch("fuse seed %d" % s["seed"], same(got, oracle_lib.fuse_search(fs)))
        mt.close()
    print("stress: %d scenes, %d skipped for a window over 1024 candidates (%d of them not predicted by the second opinion), %d mismatches" %
          (nscenes, skipped, unpredicted, bad))
    return bad or unpredicted


# ---- the committed scenes ------------------------------------------------------------------------------------------------------------
def through_frames(scene, frames):
    """the scene's problems with every searched side in a DeviceFrame: one handle per distinct side, published here"""
    from pointslot_amd.frame import DeviceFrame
    out = []
    for pr in scene["problems"]:
        T = pr["train"]
        if id(T) not in frames:
            n = len(T["x"])
            F = frames[id(T)] = DeviceFrame(max(n, 1))
            F.publish(dict(T, angle=T.get("angle", np.zeros(n, np.float32))), T["u_right"], T["desc"], T["grid"])
        host = {k: T[k] for k in ("occupied", "in_bbox") if k in T}
        out.append(dict(pr, train=dict(host, frame=frames[id(T)])))
    return out


def run_cases(seed, budget):
    global skipped
    import match_cases
    scenes, refs = match_cases.scenes(seed, budget), match_cases.references(seed, budget)
    mt = ORBmatcher(0.8, True)                                     # one handle for the whole run
    ncalls = 0
    for it, (scene, ref) in enumerate(zip(scenes, refs)):
        poison_lds(0xFFFFFFFF if it % 2 == 0 else 0x7FF00000)
        call = {"proj": mt.SearchByProjection, "bf": mt.SearchByBruceMatching, "fuse": mt.FuseSearch}[scene["kind"]]
        frames = {}
        for check_ori in (True, False):
            mt.mfNNratio, mt.mbCheckOrientation = scene["nnratio"], check_ori
            for how in ("host arrays", "frames") if scene["kind"] != "bf" else ("host arrays",):
                problems = scene["problems"] if how == "host arrays" else through_frames(scene, frames)
                try:
                    res = call(problems)
                except PointslotError as e:
                    if not capacity(e):
                        raise
                    skipped += 1
                    print("scene %d (%s, %s) from %s: %s" % (it, scene["kind"], scene["family"], how, str(e)[:80])); continue
                ncalls += 1
                for p, (got, r) in enumerate(zip(res, ref)):
                    msg = same(got, r["oracle"][check_ori])
                    if msg:
                        mismatch("match seed %d scene %d (%s, %s) problem %d mode %s nnratio %g ori %s from %s" %
                                 (seed, it, scene["kind"], scene["family"], p, r["mode"], scene["nnratio"], check_ori, how), msg)
        for F in frames.values():
            F.close()
    mt.close()
    print("stress cases: seed %d, %d scenes, %d calls, %d skipped for a window over 1024 candidates, %d mismatches" % (seed, len(scenes), ncalls, skipped, bad))
    return bad or skipped


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--cases":
        import sweep_cases
        seed = int(args[1]) if len(args) > 1 else sweep_cases.COMMITTED["match"][0]
        budget = int(args[2]) if len(args) > 2 else sweep_cases.COMMITTED["match"][1]
        sys.exit(1 if run_cases(seed, budget) else 0)
    sys.exit(1 if run_random(int(args[0]) if args else 1, int(args[1]) if len(args) > 1 else 60) else 0)
