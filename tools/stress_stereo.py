"""Randomised parity sweep of the stereo matcher against the CPU checker, bit for bit (developer tool, run on the GPU box): the scenes of
tests/stereo_cases.py through the three call forms - ComputeStereoMatches on two handles, extract_batch + stereo_match_batch +
stereo_fetch / stereo_fetch_frames on one, ComputeObjStereoMatches on hand-built key sets - over image sizes, level counts, scale
factors, quotas and disparity ranges (maxD below one pixel .. beyond the image width), with blank images, the left image on both sides
and one batch of ten pairs.  Every scene is inside the documented limits: an error is a failure.  After each key-set call the frame's
own ComputeStereoMatches results must still fetch unchanged.  usage: stress_stereo.py [seed [budget]]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
from pointslot_amd._lib import poison_lds
import stereo_cases
import sweep_cases
from pointslot_amd.extractor import ORBextractor, ComputeStereoMatches, ComputeObjStereoMatches

seed = int(sys.argv[1]) if len(sys.argv) > 1 else sweep_cases.COMMITTED["stereo"][0]
budget = int(sys.argv[2]) if len(sys.argv) > 2 else sweep_cases.COMMITTED["stereo"][1]
bad = ncalls = 0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differs(got, ref):
    """got: (uRight, depth, kept or None) of the device; ref: (kept, uRight, depth) of the oracle.  None, or what differs."""
    ur, dp, kept = got
    if len(ur) != len(ref[1]) or len(dp) != len(ref[2]):
        return "%d / %d values for %d left keys" % (len(ur), len(dp), len(ref[1]))
    if kept is not None and kept != ref[0]:
        return "kept %d, oracle %d" % (kept, ref[0])
    nu, nd = int((bits(ur) != bits(ref[1])).sum()), int((bits(dp) != bits(ref[2])).sum())
    return "%d uRight and %d depth values differ" % (nu, nd) if nu or nd else None


def check(what, it, scene, pair, got, ref):
    global bad, ncalls
    ncalls += 1
    msg = differs(got, ref)
    if msg:
        bad += 1
        print("MISMATCH stereo seed %d scene %d (%s, %s) pair %d, %s: %dx%d levels %d scale %.1f nfeatures %d mb %.6g mbf %.6g: %s" %
              (seed, it, scene["kind"], scene["pair_kinds"][pair], pair, what, scene["w"], scene["h"], scene["levels"], scene["scale"],
               scene["nfeatures"], scene["mb"], scene["mbf"], msg))


def handle(scene, max_batch=1):
    return ORBextractor(scene["nfeatures"], scene["scale"], scene["levels"], stereo_cases.INI_TH, stereo_cases.MIN_TH, max_batch=max_batch)


for it, scene in enumerate(stereo_cases.scenes(seed, budget)):
    poison_lds(0xFFFFFFFF if it % 2 == 0 else 0x7FF00000)      # uninitialised-LDS reads become deterministic failures
    refs = stereo_cases.oracle_of(scene)
    mb, mbf, npairs = scene["mb"], scene["mbf"], len(scene["pairs"])
    if scene["kind"] == "image":
        # one interleaved batch on one handle: the single fetch and the bulk fetch
        exb = handle(scene, 2 * npairs)
        exb.extract_batch([im for pair in scene["pairs"] for im in pair])
        exb.stereo_match_batch(npairs, mb, mbf)
        frames = exb.stereo_fetch_frames(npairs)
        for p in range(npairs):
            check("stereo_fetch", it, scene, p, exb.stereo_fetch(p), refs[p])
            check("stereo_fetch_frames", it, scene, p, (frames[p][2], frames[p][3], frames[p][4]), refs[p])
        exb.close()
    # two handles, as the reference's Frame has them; of the batch the pairs of its second grid row, a blank one and its neighbour
    for p in (range(npairs) if npairs == 1 else (4, 5, 9)):
        exl, exr = handle(scene), handle(scene)
        left, right = scene["pairs"][p]
        exl(left); exr(right)
        if scene["kind"] == "image" or it % 2 == 0:              # (every other key-set scene meets a handle without frame results)
            ur, dp = ComputeStereoMatches(exl, exr, mb, mbf)
            frame = exl.stereo_fetch(0)
            if scene["kind"] == "image":
                check("ComputeStereoMatches", it, scene, p, (ur, dp, None), refs[p])
                check("stereo_fetch after ComputeStereoMatches", it, scene, p, frame, refs[p])
        else:
            frame = None
        if scene["kind"] == "keys":
            for again in range(2):                               # the second call finds the first one's buffers
                got = ComputeObjStereoMatches(exl, exr, scene["kps_l"], scene["desc_l"], scene["kps_r"], scene["desc_r"], mb, mbf)
                check("ComputeObjStereoMatches", it, scene, p, got, refs[p])
                if frame is not None:
                    check("the frame's results after ComputeObjStereoMatches", it, scene, p, exl.stereo_fetch(0), (frame[2], frame[0], frame[1]))
        exl.close(); exr.close()
print("stress_stereo: seed %d, %d scenes, %d comparisons, %d mismatches" % (seed, budget, ncalls, bad))
sys.exit(1 if bad else 0)
