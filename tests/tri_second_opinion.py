"""An independent statement of LocalMapping::CreateNewMapPoints' data-parallel part, written from the reference's text in plain
Python / numpy - test infrastructure, no code shared with the library:

  create_new_map_points       /root/reference/src/LocalMapping.cc:414-707 (the loop over the neighbours, the baseline gate :461-475,
                              the per-match triangulation and its gates :519-684)
  search_for_triangulation    /root/reference/src/ORBmatcher.cc:783-979 (+ CheckDistEpipolarLine :261-278, ComputeThreeMaxima :2658-2699)
  unproject_stereo            /root/reference/src/KeyFrame.cc:711-727
  the feature vector          Thirdparty/DBoW2/DBoW2/FeatureVector.cpp:31-45 (a std::map node -> features in ascending index)

It is sequential, one neighbour after the other, one feature after the other: the candidate loop keeps the reference's
`dist > bestDist` test and its running bestDist (only the gate VALUES of a node's candidates are formed as arrays beforehand), so
the library's "least distance, highest index" rule is checked against the loop it was derived from.  Everything the reference
holds as `float` is a numpy float32 and every operation on it is rounded on its own; cv::Mat products, Mat::dot and cv::norm
accumulate in double and round once (the project's standing choice, tests/match_second_opinion.py:17-21).  Two places follow
include/pointslot_hip.h's modelling choices: the null vector of A is np.linalg.svd on the float64 copy of A, divided by its
fourth component in float64 and rounded once per coordinate; the stereo cosine is math.cos(2 * math.atan2(mb / 2, depth)) on the
float32 mb / 2 and depth, rounded once.

Per triangulated pair the result also says how well-posed the comparison is: sigma1 / sigma3 of A, and whether the verdict is
STABLE - the same for x3D and for each of its 26 neighbours at +-1 float32 ulp per coordinate, and the same branch for the
stereo cosine at +-1 ulp."""
import math

import numpy as np

from match_second_opinion import three_maxima, _rot_bin

F32, F64 = np.float32, np.float64
TH_LOW, HISTO_LENGTH = 50, 30
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)
CREATED, NO_MATCH, OCCUPIED, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE_RATIO, SKIPPED = range(12)


def _f(v):
    return np.asarray(v, F32)


def _dot3d(a, b):
    """a . b of float32 vectors the way cv::gemm / Mat::dot / cv::norm form it: products and sum in double, left to right"""
    a = np.asarray(a, F64); b = np.asarray(b, F64)
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def feature_vector(node):
    fv = {}
    for i, v in enumerate(np.asarray(node)):
        if v >= 0:
            fv.setdefault(int(v), []).append(i)    # addFeature: push_back in feature order
    return fv


def search_for_triangulation(kf1, kf2, F12, only_stereo, check_ori, occupied1=None):
    """-> (nmatches, vMatches12 as an int32 array).  occupied1: pKF1->GetMapPoint(idx1) != NULL (default kf1["occupied"])"""
    N1 = len(kf1["node"])
    occ1 = np.asarray(kf1["occupied"] if occupied1 is None else occupied1)
    occ2 = np.asarray(kf2["occupied"])
    F = _f(F12).reshape(3, 3)
    R2, t2, Cw = _f(kf2["R"]).reshape(3, 3), _f(kf2["t"]).reshape(3), _f(kf1["ow"]).reshape(3)
    fx2, fy2, cx2, cy2 = [F32(v) for v in kf2["K8"][:4]]
    C2 = [F32(F32(_dot3d(R2[r], Cw)) + t2[r]) for r in range(3)]
    invz = F32(F32(1.0) / C2[2])
    ex = F32(F32(F32(fx2 * C2[0]) * invz) + cx2)
    ey = F32(F32(F32(fy2 * C2[1]) * invz) + cy2)
    x1, y1, ur1, d1, a1 = _f(kf1["x"]), _f(kf1["y"]), _f(kf1["u_right"]), np.asarray(kf1["desc"], np.uint8).reshape(-1, 32), _f(kf1["angle"])
    x2, y2, ur2, d2, a2 = _f(kf2["x"]), _f(kf2["y"]), _f(kf2["u_right"]), np.asarray(kf2["desc"], np.uint8).reshape(-1, 32), _f(kf2["angle"])
    oct2 = np.asarray(kf2["octave"])
    sf2, sg2 = _f(kf2["scale_factors"]), _f(kf2["level_sigma2"])
    fv1, fv2 = feature_vector(kf1["node"]), feature_vector(kf2["node"])
    matches = np.full(N1, -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for node in sorted(set(fv1) & set(fv2)):      # the merge walk over the two maps stops exactly at their common keys, in key order
        l2 = np.array(fv2[node])
        kx2, ky2 = x2[l2], y2[l2]
        stereo2 = ur2[l2] >= 0
        disc = F32(100.0) * sf2[oct2[l2]]
        thr = 3.84 * sg2[oct2[l2]].astype(F64)
        for idx1 in fv1[node]:
            if occ1[idx1]:
                continue
            stereo1 = ur1[idx1] >= 0
            if only_stereo and not stereo1:
                continue
            dist = _POP[np.bitwise_xor(d2[l2], d1[idx1][None, :])].sum(axis=1)
            # CheckDistEpipolarLine for every candidate of the node
            a = F32(F32(F32(x1[idx1] * F[0, 0]) + F32(y1[idx1] * F[1, 0])) + F[2, 0])
            b = F32(F32(F32(x1[idx1] * F[0, 1]) + F32(y1[idx1] * F[1, 1])) + F[2, 1])
            c = F32(F32(F32(x1[idx1] * F[0, 2]) + F32(y1[idx1] * F[1, 2])) + F[2, 2])
            num = (a * kx2 + b * ky2) + c
            den = F32(F32(a * a) + F32(b * b))
            if den == 0:
                epi_ok = np.zeros(len(l2), bool)
            else:
                epi_ok = ((num * num) / den).astype(F64) < thr
            dx, dy = ex - kx2, ey - ky2
            in_disc = (dx * dx + dy * dy) < disc
            best_dist, best_idx2 = TH_LOW, -1
            for j, idx2 in enumerate(l2):
                if occ2[idx2]:                    # vbMatched2[idx2] is never set
                    continue
                if only_stereo and not stereo2[j]:
                    continue
                if dist[j] > TH_LOW or dist[j] > best_dist:
                    continue
                if not stereo1 and not stereo2[j] and in_disc[j]:
                    continue
                if epi_ok[j]:
                    best_idx2, best_dist = int(idx2), int(dist[j])
            if best_idx2 >= 0:
                matches[idx1] = best_idx2
                nmatches += 1
                if check_ori:
                    hist[_rot_bin(a1[idx1], a2[best_idx2])].append(idx1)
    if check_ori:
        keep = three_maxima([len(h) for h in hist])
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for idx1 in hist[i]:
                matches[idx1] = -1
                nmatches -= 1
    return nmatches, matches


def unproject_stereo(kf, i):
    z = _f(kf["depth"])[i]
    assert z > 0
    fx, fy, cx, cy, invfx, invfy = [F32(v) for v in kf["K8"][:6]]
    u = _f(kf["x_raw"] if kf.get("x_raw") is not None else kf["x"])[i]
    v = _f(kf["y_raw"] if kf.get("y_raw") is not None else kf["y"])[i]
    x = F32(F32(F32(u - cx) * z) * invfx)
    y = F32(F32(F32(v - cy) * z) * invfy)
    Rwc, ow = _f(kf["R"]).reshape(3, 3).T, _f(kf["ow"]).reshape(3)
    return np.array([F32(F32(_dot3d(Rwc[r], [x, y, z])) + ow[r]) for r in range(3)], F32)


def _rays(kf, kx, ky):
    fx, fy, cx, cy, invfx, invfy = [F32(v) for v in kf["K8"][:6]]
    xn = np.array([F32(F32(kx - cx) * invfx), F32(F32(ky - cy) * invfy), F32(1.0)], F32)
    Rwc = _f(kf["R"]).reshape(3, 3).T
    return xn, np.array([F32(_dot3d(Rwc[r], xn)) for r in range(3)], F32)


def _branch(cos_rays, cs1, cs2, st1, st2):
    cs = cs2 if cs2 < cs1 else cs1               # std::min
    if cos_rays < cs and cos_rays > 0 and (st1 or st2 or F64(cos_rays) < 0.9998):
        return "svd"
    if st1 and cs1 < cs2:
        return "stereo1"
    if st2 and cs2 < cs1:
        return "stereo2"
    return "none"


def _reproj_fail(kf, X, Xd, z, kx, ky, kur, octave, mbf):
    """X float32 [m, 3] -> bool [m]"""
    R, t = _f(kf["R"]).reshape(3, 3), _f(kf["t"]).reshape(3)
    fx, fy, cx, cy = [F32(v) for v in kf["K8"][:4]]
    sigma2 = _f(kf["level_sigma2"])[octave]
    x = (_dot3d(R[0], Xd) + F64(t[0])).astype(F32)
    y = (_dot3d(R[1], Xd) + F64(t[1])).astype(F32)
    invz = (1.0 / z.astype(F64)).astype(F32)
    u = fx * x * invz + cx
    v = fy * y * invz + cy
    ex, ey = u - F32(kx), v - F32(ky)
    if not kur >= 0:
        return (ex * ex + ey * ey).astype(F64) > 5.991 * F64(sigma2)
    u_r = u - F32(mbf) * invz
    er = u_r - F32(kur)
    return (ex * ex + ey * ey + er * er).astype(F64) > 7.8 * F64(sigma2)


def gates(X, kf1, kf2, idx1, idx2, ratio_factor):
    """LocalMapping.cc:598-684 for the points X (float32 [m, 3]) -> status [m]"""
    X = np.asarray(X, F32).reshape(-1, 3)
    Xd = X.astype(F64)
    st = np.zeros(len(X), np.int64)

    def fail(cond, code):
        st[(st == 0) & cond] = code
    R1, t1, R2, t2 = _f(kf1["R"]).reshape(3, 3), _f(kf1["t"]).reshape(3), _f(kf2["R"]).reshape(3, 3), _f(kf2["t"]).reshape(3)
    with np.errstate(all="ignore"):
        z1 = (_dot3d(R1[2], Xd) + F64(t1[2])).astype(F32)
        fail(z1 <= 0, Z1)
        z2 = (_dot3d(R2[2], Xd) + F64(t2[2])).astype(F32)
        fail(z2 <= 0, Z2)
        mbf = kf1["K8"][7]                         # mpCurrentKeyFrame->mbf in both tests (:631, :658)
        fail(_reproj_fail(kf1, X, Xd, z1, _f(kf1["x"])[idx1], _f(kf1["y"])[idx1], _f(kf1["u_right"])[idx1], int(kf1["octave"][idx1]), mbf), REPROJ1)
        fail(_reproj_fail(kf2, X, Xd, z2, _f(kf2["x"])[idx2], _f(kf2["y"])[idx2], _f(kf2["u_right"])[idx2], int(kf2["octave"][idx2]), mbf), REPROJ2)
        n1 = X - _f(kf1["ow"]).reshape(1, 3)
        n2 = X - _f(kf2["ow"]).reshape(1, 3)
        dist1 = np.sqrt(_dot3d(n1, n1)).astype(F32)
        dist2 = np.sqrt(_dot3d(n2, n2)).astype(F32)
        fail((dist1 == 0) | (dist2 == 0), ZERO_DIST)
        ratio_dist = dist2 / dist1
        ratio_octave = F32(_f(kf1["scale_factors"])[int(kf1["octave"][idx1])] / _f(kf2["scale_factors"])[int(kf2["octave"][idx2])])
        rf = F32(ratio_factor)
        fail((ratio_dist * rf < ratio_octave) | (ratio_dist > ratio_octave * rf), SCALE_RATIO)
    return st


def _ulp_neighbours(X):
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                out.append([np.nextafter(X[c], F32(np.inf) * F32(d), dtype=F32) if d else X[c] for c, d in enumerate((dx, dy, dz))])
    return np.array(out, F32)


def triangulate_pair(kf1, kf2, idx1, idx2, ratio_factor):
    """-> dict(status, x3d, kind, ratio, stable)"""
    kx1, ky1, kur1 = _f(kf1["x"])[idx1], _f(kf1["y"])[idx1], _f(kf1["u_right"])[idx1]
    kx2, ky2, kur2 = _f(kf2["x"])[idx2], _f(kf2["y"])[idx2], _f(kf2["u_right"])[idx2]
    st1, st2 = bool(kur1 >= 0), bool(kur2 >= 0)
    xn1, ray1 = _rays(kf1, kx1, ky1)
    xn2, ray2 = _rays(kf2, kx2, ky2)
    cos_rays = F32(_dot3d(ray1, ray2) / (math.sqrt(_dot3d(ray1, ray1)) * math.sqrt(_dot3d(ray2, ray2))))
    cs1 = cs2 = F32(cos_rays + F32(1.0))
    moved = None
    if st1:
        cs1 = F32(math.cos(2.0 * math.atan2(float(F32(F32(kf1["K8"][6]) / F32(2.0))), float(_f(kf1["depth"])[idx1]))))
        moved = 1
    elif st2:
        cs2 = F32(math.cos(2.0 * math.atan2(float(F32(F32(kf2["K8"][6]) / F32(2.0))), float(_f(kf2["depth"])[idx2]))))
        moved = 2
    kind = _branch(cos_rays, cs1, cs2, st1, st2)
    stable = True
    for d in (-np.inf, np.inf):                    # the stereo cosine at +-1 ulp must take the same branch
        if moved == 1:
            stable &= _branch(cos_rays, np.nextafter(cs1, F32(d), dtype=F32), cs2, st1, st2) == kind
        elif moved == 2:
            stable &= _branch(cos_rays, cs1, np.nextafter(cs2, F32(d), dtype=F32), st1, st2) == kind
    res = dict(status=LOW_PARALLAX, x3d=np.zeros(3, F32), kind=kind, ratio=0.0, stable=bool(stable))
    if kind == "none":
        return res
    if kind == "svd":
        T1 = np.concatenate([_f(kf1["R"]).reshape(3, 3), _f(kf1["t"]).reshape(3, 1)], 1)
        T2 = np.concatenate([_f(kf2["R"]).reshape(3, 3), _f(kf2["t"]).reshape(3, 1)], 1)
        A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]]).astype(F32)
        _, s, vt = np.linalg.svd(A.astype(F64))
        res["ratio"] = float(s[0] / s[2]) if s[2] > 0 else float("inf")
        v = vt[3]
        if F32(v[3]) == 0:
            res["status"] = W_ZERO
            return res
        X = (v[:3] / v[3]).astype(F32)
    elif kind == "stereo1":
        X = unproject_stereo(kf1, idx1)
    else:
        X = unproject_stereo(kf2, idx2)
    st = gates(_ulp_neighbours(X), kf1, kf2, idx1, idx2, ratio_factor)
    res["status"] = int(st[13])                    # the centre of the 3 x 3 x 3 neighbourhood
    res["x3d"] = X
    res["stable"] = bool(stable and np.all(st == st[13]))
    return res


def create_new_map_points(pr):
    """pr: a problem dict as pointslot_amd.matcher.ORBmatcher.CreateNewMapPoints takes it -> dict(match [k, n1], nmatches [k],
    status [k, n1], x3d [k, n1, 3], nnew, pairs: [dict(i, idx1, idx2, kind, ratio, stable, status)])"""
    kf1, nb = pr["kf1"], pr["kf2"]
    k, n1 = len(nb), len(kf1["node"])
    tri, chain = bool(pr.get("triangulate", 1)), bool(pr.get("chain", 1))
    occ1 = np.array(kf1["occupied"], np.uint8).copy()
    match = np.full((k, n1), -1, np.int32)
    nmatches = np.zeros(k, np.int32)
    status = np.full((k, n1), NO_MATCH, np.uint8)
    x3d = np.zeros((k, n1, 3), F32)
    pairs = []
    nnew = 0
    for i, kf2 in enumerate(nb):
        if tri:
            base = _f(kf2["ow"]).reshape(3) - _f(kf1["ow"]).reshape(3)
            baseline = F32(math.sqrt(_dot3d(base, base)))
            if baseline < F32(kf2["K8"][6]):       # !mbMonocular: baseline < pKF2->mb
                status[i, :] = SKIPPED
                continue
        seen = occ1 if chain else np.asarray(kf1["occupied"], np.uint8)
        status[i, seen != 0] = OCCUPIED
        nmatches[i], match[i] = search_for_triangulation(kf1, kf2, np.asarray(pr["f12"])[i], bool(pr.get("only_stereo")),
                                                         bool(pr.get("check_orientation", 1)), seen.copy())
        if not tri:
            continue
        for idx1 in np.nonzero(match[i] >= 0)[0]:
            r = triangulate_pair(kf1, kf2, int(idx1), int(match[i, idx1]), pr["ratio_factor"])
            status[i, idx1] = r["status"]
            x3d[i, idx1] = r["x3d"]
            pairs.append(dict(i=i, idx1=int(idx1), idx2=int(match[i, idx1]), **{a: r[a] for a in ("kind", "ratio", "stable", "status")}))
            if r["status"] == CREATED:
                occ1[idx1] = 1                     # mpCurrentKeyFrame->AddMapPoint(pMP, idx1)
                nnew += 1
    out = dict(match=match, nmatches=nmatches, nnew=nnew, pairs=pairs)
    if tri:
        out.update(status=status, x3d=x3d)
    return out
