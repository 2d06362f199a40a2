"""An independent statement of the four loop-closure / relocalisation projection matchers, written from the reference's text in plain
Python / numpy - test infrastructure, no code shared with the library.

  search_by_projection_sim3      /root/reference/src/ORBmatcher.cc:413-526    SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
  fuse_sim3                      :1262-1385   Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)  (the search half)
  search_by_projection_keyframe  :2529-2656   SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
  search_by_sim3                 :1387-1611   SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
  KeyFrame::GetFeaturesInArea / IsInImage   /root/reference/src/KeyFrame.cc:665-709;  MapPoint::PredictScale  MapPoint.cc:515-547

Every float of the reference is a numpy.float32 here and every operation on it is rounded on its own; cv::Mat products, Mat::dot and
cv::norm accumulate in double (tests/match_second_opinion.py, accumulate="double").  The problems are the dicts pointslot_amd.matcher
takes (ORBmatcher.KfSearch / SearchBySim3): the pose arrives decomposed (R, t, ow), the map data model as flags.  The two
order-dependent members are the reference's sequential loops.  Besides the results every function reports, per query, the gate that
ended it and the FP64 value log(ratio) / logScale PredictScale rounds up (NaN where the query never got there) - the input condition
of the GPU comparison is stated on those (tests/test_kfsearch_cpu.py)."""
import math

import numpy as np

from match_second_opinion import Grid, descriptor_distance, three_maxima, _c_round, _mat3_vec_plus

F32 = np.float32
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30
INT_MAX = 2 ** 31 - 1
GATES = {0: ("invalid", "depth", "image", "distance", "angle", "empty", "nomatch", "match"),
         1: ("invalid", "depth", "image", "distance", "angle", "empty", "nomatch", "match"),
         2: ("invalid", "image", "distance", "empty", "nomatch", "match"),
         3: ("invalid", "depth", "image", "distance", "empty", "nomatch", "match")}


def _pose(R, t):
    T = np.zeros((4, 4), F32)
    T[:3, :3] = np.asarray(R, F32).reshape(3, 3)
    T[:3, 3] = np.asarray(t, F32).reshape(3)
    return T


def _norm(p):
    """cv::norm of a float 3-vector: squares and sum in double, the caller stores the root in a float"""
    return F32(math.sqrt(float(p[0]) * float(p[0]) + float(p[1]) * float(p[1]) + float(p[2]) * float(p[2])))


def _predict_scale(max_dist, dist, log_scale, n_levels):
    """-> (level, the FP64 quotient, the float ratio)"""
    ratio = F32(F32(max_dist) / F32(dist))
    with np.errstate(all="ignore"):
        logv = float(np.log(np.float64(ratio))) / float(F32(log_scale))
    if math.isnan(logv):
        return 0, logv, ratio
    lvl = int(math.ceil(logv)) if math.isfinite(logv) else (0 if logv < 0 else n_levels - 1)
    return (0 if lvl < 0 else (n_levels - 1 if lvl >= n_levels else lvl)), logv, ratio


def _keyframe_area(g, u, v, r):
    """KeyFrame::GetFeaturesInArea: no level filter inside"""
    return g.features_in_area(u, v, r, None, -1, -1)


def _project_kf(xc, yc, zc, fx, fy, cx, cy):
    """invz = 1 / z; x = xc * invz; u = fx * x + cx  (:454-459)"""
    with np.errstate(all="ignore"):
        invz = F32(F32(1.0) / zc)
        return F32(F32(fx * F32(xc * invz)) + cx), F32(F32(fy * F32(yc * invz)) + cy)


def _in_image(u, v, b):
    return bool(u >= b[0] and u < b[1] and v >= b[2] and v < b[3])


class _Side:
    def __init__(self, T):
        self.n = len(T["x"])
        self.grid = Grid(T["x"], T["y"], T["grid"])
        self.octave = np.asarray(T["octave"])
        self.desc = np.asarray(T["desc"], np.uint8).reshape(-1, 32)
        self.angle = np.asarray(T.get("angle", np.zeros(self.n)), F32)


def _window_best(side, cand, desc, lo, hi, blocked, start):
    best, bidx = start, -1
    for j in cand:
        if blocked is not None and blocked[j]:
            continue
        if side.octave[j] < lo or side.octave[j] > hi:
            continue
        d = descriptor_distance(desc, side.desc[j])
        if d < best:
            best, bidx = d, j
    return best, bidx


def _sim3_overload(pr, mode):
    """modes 0 and 1 share everything up to the candidate loop"""
    S = _Side(pr["train"])
    q = pr["query"]
    T = _pose(pr["R"], pr["t"])
    ow = np.asarray(pr["ow"], F32)
    fx, fy, cx, cy = [F32(v) for v in pr["K4"]]
    b = [F32(v) for v in pr["bounds"]]
    sf, th = np.asarray(pr["scale_factors"], F32), F32(pr["th"])
    valid, pos, nor = np.asarray(q["valid"]), np.asarray(q["pos"], F32).reshape(-1, 3), np.asarray(q["normal"], F32).reshape(-1, 3)
    mind, maxd, qdesc = np.asarray(q["min_dist"], F32), np.asarray(q["max_dist"], F32), np.asarray(q["desc"], np.uint8).reshape(-1, 32)
    m = len(valid)
    blocked = np.asarray(pr["train"].get("occupied", np.zeros(S.n, np.uint8))).astype(bool).copy() if mode == 0 else None
    match = np.full(S.n, -1, np.int32)
    best_idx, best_dist = np.full(m, -1, np.int32), np.full(m, 256, np.int32)
    gate, logv, ratio = ["invalid"] * m, np.full(m, np.nan), np.full(m, np.nan, F32)
    nm = 0
    for i in range(m):
        if not valid[i]:
            continue
        xc, yc, zc = _mat3_vec_plus(T, pos[i], "double")
        if zc < 0.0:
            gate[i] = "depth"; continue
        u, v = _project_kf(xc, yc, zc, fx, fy, cx, cy)
        if not _in_image(u, v, b):
            gate[i] = "image"; continue
        PO = [F32(pos[i][k] - ow[k]) for k in range(3)]
        dist = _norm(PO)
        if dist < F32(F32(0.8) * mind[i]) or dist > F32(F32(1.2) * maxd[i]):
            gate[i] = "distance"; continue
        dotn = float(PO[0]) * float(nor[i][0]) + float(PO[1]) * float(nor[i][1]) + float(PO[2]) * float(nor[i][2])
        if dotn < 0.5 * float(dist):
            gate[i] = "angle"; continue
        lvl, logv[i], ratio[i] = _predict_scale(maxd[i], dist, pr["log_scale_factor"], int(pr["n_levels"]))
        cand = _keyframe_area(S.grid, u, v, F32(th * sf[lvl]))
        if not cand:
            gate[i] = "empty"; continue
        best, bidx = _window_best(S, cand, qdesc[i], lvl - 1, lvl, blocked, 256 if mode == 0 else INT_MAX)
        if best <= TH_LOW:
            gate[i] = "match"
            nm += 1
            if mode == 0:
                match[bidx] = i
                blocked[bidx] = True
            else:
                best_idx[i] = bidx
        else:
            gate[i] = "nomatch"
        if mode == 1 and bidx >= 0:
            best_dist[i] = best
    out = dict(nmatches=nm, gate=gate, logv=logv, ratio=ratio)
    if mode == 0:
        out["match_of_train"] = match
    else:
        out.update(best_idx=best_idx, best_dist=best_dist)
    return out


def search_by_projection_sim3(pr):
    return _sim3_overload(pr, 0)


def fuse_sim3(pr):
    return _sim3_overload(pr, 1)


def search_by_projection_keyframe(pr, check_ori=True, factor=None):
    """factor: the histogram factor; None = the overload's own 1.0f / HISTO_LENGTH (:2541).  The tracking overloads use
    HISTO_LENGTH / 360.0f - pass that to see what reusing theirs would give."""
    S = _Side(pr["train"])
    q = pr["query"]
    T = _pose(pr["R"], pr["t"])
    ow = np.asarray(pr["ow"], F32)
    fx, fy, cx, cy = [F32(v) for v in pr["K4"]]
    minx, maxx, miny, maxy = [F32(v) for v in pr["bounds"]]
    sf, th = np.asarray(pr["scale_factors"], F32), F32(pr["th"])
    orb_dist = int(pr.get("th_dist", TH_HIGH))
    factor = F32(F32(1.0) / F32(HISTO_LENGTH)) if factor is None else F32(factor)
    valid, pos = np.asarray(q["valid"]), np.asarray(q["pos"], F32).reshape(-1, 3)
    mind, maxd, qdesc = np.asarray(q["min_dist"], F32), np.asarray(q["max_dist"], F32), np.asarray(q["desc"], np.uint8).reshape(-1, 32)
    qang = np.asarray(q.get("angle", np.zeros(len(valid))), F32)
    m = len(valid)
    blocked = np.asarray(pr["train"].get("occupied", np.zeros(S.n, np.uint8))).astype(bool).copy()
    match = np.full(S.n, -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    gate, logv, ratio = ["invalid"] * m, np.full(m, np.nan), np.full(m, np.nan, F32)
    nm = 0
    for i in range(m):
        if not valid[i]:
            continue
        xc, yc, zc = _mat3_vec_plus(T, pos[i], "double")
        with np.errstate(all="ignore"):
            invzc = F32(1.0 / np.float64(zc))
            u = F32(F32(F32(fx * xc) * invzc) + cx)
            v = F32(F32(F32(fy * yc) * invzc) + cy)
        # (a non-finite u or v is undefined behaviour in the reference; the modelling choice: outside the image)
        if not (np.isfinite(u) and np.isfinite(v)) or u < minx or u > maxx or v < miny or v > maxy:
            gate[i] = "image"; continue
        dist = _norm([F32(pos[i][k] - ow[k]) for k in range(3)])
        if dist < F32(F32(0.8) * mind[i]) or dist > F32(F32(1.2) * maxd[i]):
            gate[i] = "distance"; continue
        lvl, logv[i], ratio[i] = _predict_scale(maxd[i], dist, pr["log_scale_factor"], int(pr["n_levels"]))
        cand = S.grid.features_in_area(u, v, F32(th * sf[lvl]), S.octave, lvl - 1, lvl + 1)
        if not cand:
            gate[i] = "empty"; continue
        best, bidx = 256, -1
        for j in cand:
            if blocked[j]:
                continue
            d = descriptor_distance(qdesc[i], S.desc[j])
            if d < best:
                best, bidx = d, j
        if best <= orb_dist:
            gate[i] = "match"
            match[bidx] = i
            blocked[bidx] = True
            nm += 1
            if check_ori:
                rot = F32(qang[i] - S.angle[bidx])
                if rot < 0.0:
                    rot = F32(rot + F32(360.0))
                bn = _c_round(F32(rot * factor))
                if bn == HISTO_LENGTH:
                    bn = 0
                hist[bn].append(bidx)
        else:
            gate[i] = "nomatch"
    if check_ori:
        keep = three_maxima([len(h) for h in hist])
        for bn in range(HISTO_LENGTH):
            if bn in keep:
                continue
            for j in hist[bn]:
                match[j] = -2
                nm -= 1
    return dict(nmatches=nm, match_of_train=match, gate=gate, logv=logv, ratio=ratio, bins=[len(h) for h in hist])


def _sim3_direction(Q, S_other, other, T1, T2, K4, th):
    """the points of keyframe Q into the features of the other keyframe: vnMatch, gates, logv, ratio"""
    fx, fy, cx, cy = [F32(v) for v in K4]
    b = [F32(v) for v in other["bounds"]]
    sf = np.asarray(other["scale_factors"], F32)
    has, already = np.asarray(Q["has_point"]), np.asarray(Q.get("already", np.zeros(len(Q["has_point"]))))
    pos = np.asarray(Q["pos"], F32).reshape(-1, 3)
    mind, maxd, pdesc = np.asarray(Q["min_dist"], F32), np.asarray(Q["max_dist"], F32), np.asarray(Q["point_desc"], np.uint8).reshape(-1, 32)
    n = len(has)
    vn = np.full(n, -1, np.int32)
    gate, logv, ratio = ["invalid"] * n, np.full(n, np.nan), np.full(n, np.nan, F32)
    for i in range(n):
        if not has[i] or already[i]:
            continue
        p1 = _mat3_vec_plus(T1, pos[i], "double")
        xc, yc, zc = _mat3_vec_plus(T2, p1, "double")
        if zc < 0.0:
            gate[i] = "depth"; continue
        u, v = _project_kf(xc, yc, zc, fx, fy, cx, cy)
        if not _in_image(u, v, b):
            gate[i] = "image"; continue
        dist = _norm([xc, yc, zc])
        if dist < F32(F32(0.8) * mind[i]) or dist > F32(F32(1.2) * maxd[i]):
            gate[i] = "distance"; continue
        lvl, logv[i], ratio[i] = _predict_scale(maxd[i], dist, other["log_scale_factor"], int(other["n_levels"]))
        cand = _keyframe_area(S_other.grid, u, v, F32(F32(th) * sf[lvl]))
        if not cand:
            gate[i] = "empty"; continue
        best, bidx = _window_best(S_other, cand, pdesc[i], lvl - 1, lvl, None, INT_MAX)
        if best <= TH_HIGH:
            vn[i] = bidx
            gate[i] = "match"
        else:
            gate[i] = "nomatch"
    return vn, gate, logv, ratio


def search_by_sim3(pr):
    from pointslot_amd.matcher import sim3_pair
    kf1, kf2 = pr["kf1"], pr["kf2"]
    sr12, t12, sr21, t21 = (pr["sr12"], pr["t12"], pr["sr21"], pr["t21"]) if "sr12" in pr else sim3_pair(pr["s12"], pr["R12"], pr["t12"])
    S1, S2 = _Side(kf1), _Side(kf2)
    m1, g1, l1, r1 = _sim3_direction(kf1, S2, kf2, _pose(kf1["R"], kf1["t"]), _pose(sr21, t21), pr["K4"], pr["th"])
    m2, g2, l2, r2 = _sim3_direction(kf2, S1, kf1, _pose(kf2["R"], kf2["t"]), _pose(sr12, t12), pr["K4"], pr["th"])
    m12 = np.full(S1.n, -1, np.int32)
    nfound = 0
    for i1 in range(S1.n):
        idx2 = m1[i1]
        if idx2 >= 0 and m2[idx2] == i1:
            m12[i1] = idx2
            nfound += 1
    return dict(nfound=nfound, match12=m12, match1=m1, match2=m2, gate=g1 + g2, logv=np.concatenate([l1, l2]), ratio=np.concatenate([r1, r2]))


def run(pr):
    """a ps_kf_search problem by its mode"""
    mode = int(pr["mode"])
    if mode == 2:
        return search_by_projection_keyframe(pr, bool(pr.get("check_orientation", True)))
    return _sim3_overload(pr, mode)
