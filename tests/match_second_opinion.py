"""An independent statement of the four order-dependent matchers, written from the reference's text in plain Python / numpy - test
infrastructure, no code shared with oracle/ (the pixel stages had a second author since r02, the greedy matchers - where a
single-author slip is most likely - had property tests only).

  search_by_bruce_matching      /root/reference/src/ORBmatcher.cc:2043-2155 (+ ComputeThreeMaxima :2658-2699, DescriptorDistance :2704-2720)
  search_by_projection_frame    :1613-1756   SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
  search_by_projection_points   :68-155      SearchByProjection(Frame& F, const vector<MapPoint*>&, th)
                                :157-248     SearchByProjection(Frame& F, nOrder, const vector<MapObjectPoint*>&, th)   (object=True)
  Frame::GetFeaturesInArea / GetObjectFeaturesInArea   /root/reference/src/Frame.cc:1808-1861, 1892-1951
  Frame::PosInGrid + AssignFeaturesToGrid              :2027-2037, 1636-1656 (a cell's list is in keypoint order)

Everything the reference holds as `float` is a numpy float32 here and every operation on it is rounded to float32 on its own; what the
reference leaves to the map data model comes in as flags, exactly as the C-ABI takes it (`occupied[j]`: the slot holds a point with
Observations() > 0; `observed[i]`: the candidate point has Observations() > 0, so its assignment blocks the slot for later candidates -
an unobserved one can be overwritten, "last assignment wins", and both count as matches).

One modelling question this file makes explicit: the camera-frame point of the frame-to-frame search is the cv::Mat expression
`Rcw*x3Dw+tcw` on CV_32F matrices.  `accumulate="double"` forms the three products and their sum in double and rounds once (cv::gemm's
general path, the restatement's choice); `accumulate="float"` rounds every product and every partial sum to float32 (the 3 x 3 small-matrix
path gemm takes for flags == 0 in OpenCV 2.4 / 3.x).  The results differ by at most an ulp of u, v; the tests run both and report whether a
match changes."""
import math

import numpy as np

F32 = np.float32
TH_HIGH, TH_LOW, TH_HIGH_FORDYNAMIC, HISTO_LENGTH = 100, 50, 130, 30
GRID_COLS, GRID_ROWS = 64, 48
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def descriptor_distance(a, b):
    """the SWAR popcount of the reference is a popcount: bits set in a ^ b over the 32 bytes"""
    return int(_POP[np.bitwise_xor(a, b)].sum())


def _distances(d, rows):
    """Hamming distance of descriptor d (32 bytes) to every row of `rows` [n, 32]"""
    return _POP[np.bitwise_xor(rows, d[None, :])].sum(axis=1)


def _hit(counts, gate, n=1):
    """one more (or n more) passages through `gate`; counts is None when nobody is counting"""
    if counts is not None and n:
        counts[gate] = counts.get(gate, 0) + n


def three_maxima(sizes, counts=None):
    """ComputeThreeMaxima on the bins' sizes -> (ind1, ind2, ind3)"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3 = s
            ind3 = i
    if F32(max2) < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif F32(max3) < F32(0.1) * F32(max1):
        ind3 = -1
    if counts is not None and max1 > 0:
        _hit(counts, "hist_kept_%d" % sum(k >= 0 for k in (ind1, ind2, ind3)))
        if F32(max2) == F32(0.1) * F32(max1) or F32(max3) == F32(0.1) * F32(max1):
            _hit(counts, "hist_on_tenth_boundary")
        if max2 == max1 or (max3 == max2 and max2 > 0):
            _hit(counts, "hist_equal_bins")
    return ind1, ind2, ind3


def _c_round(v):
    """C round(): half away from zero"""
    return int(math.floor(abs(float(v)) + 0.5)) * (1 if v >= 0 else -1)


def _rot_bin(angle_from, angle_to, counts=None):
    rot = F32(angle_from) - F32(angle_to)
    if rot < 0.0:
        rot = F32(rot + F32(360.0))
    b = _c_round(F32(rot * F32(F32(HISTO_LENGTH) / F32(360.0))))
    if b == HISTO_LENGTH:
        _hit(counts, "bin_wrap_30")
    return 0 if b == HISTO_LENGTH else b


def _rotation_check(hist, out, mark, counts):
    """the tail of the three histogram matchers: every match outside the kept bins gets `mark`; -> the number removed"""
    keep = three_maxima([len(h) for h in hist], counts)
    removed = 0
    for b in range(HISTO_LENGTH):
        if b in keep:
            continue
        for j in hist[b]:
            out[j] = mark
            removed += 1
    _hit(counts, "removed_by_rotation", removed)
    return removed


def search_by_bruce_matching(p, nnratio, check_ori, counts=None):
    """-> (nmatches, query_of_train[nt]); a train's entry is the index of the last-frame point it was given to, -1 = NULL.
    counts (a dict) receives how often each gate was passed; "rescan" is a statement about the device's eight-key lists (the global
    best is within TH_LOW, more than eight trains, fewer than two of the eight smallest (distance, index) keys still untaken)"""
    qd, td = np.asarray(p["q_desc"], np.uint8).reshape(-1, 32), np.asarray(p["t_desc"], np.uint8).reshape(-1, 32)
    qa, ta, qv = np.asarray(p["q_angle"], F32), np.asarray(p["t_angle"], F32), np.asarray(p["q_valid"])
    nt = len(td)
    out = [-1] * nt
    taken = np.zeros(nt, bool)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nm = 0
    for i in range(len(qd)):
        if not qv[i]:
            _hit(counts, "invalid")
            continue
        best1, best2, bidx = 256, 256, -1
        if nt:
            d = _distances(qd[i], td)
            if counts is not None:
                _count_bruteforce_query(counts, d, taken)
            # the scan in train order, skipping the trains already given away: best = FIRST minimum, second = best of the rest
            for j in np.nonzero(~taken)[0]:
                dj = int(d[j])
                if dj < best1:
                    best2, best1, bidx = best1, dj, int(j)
                elif dj < best2:
                    best2 = dj
        if counts is not None and bidx >= 0:
            _count_decision(counts, best1, best2, TH_LOW, F32(best1) >= F32(nnratio) * F32(best2), F32(best1) == F32(nnratio) * F32(best2))
        if best1 <= TH_LOW and F32(best1) < F32(nnratio) * F32(best2):
            if counts is not None:
                _hit(counts, "accepted")
                _hit(counts, "accepted_not_first_choice", int(bidx != int(np.argmin(d))))
            out[bidx] = i
            taken[bidx] = True
            if check_ori:
                hist[_rot_bin(qa[i], ta[bidx], counts)].append(bidx)
            nm += 1
    if check_ori:
        nm -= _rotation_check(hist, out, -1, counts)
    return nm, np.array(out, np.int32) if nt else np.zeros(0, np.int32)


def _count_decision(counts, best, best2, limit, ratio_fails, ratio_equal):
    """the gates between a query's best surviving candidate and its acceptance that all the matchers share"""
    _hit(counts, "best_eq_limit", int(best == limit))
    _hit(counts, "best_eq_limit_plus_1", int(best == limit + 1))
    _hit(counts, "over_limit", int(best > limit))
    if best <= limit and ratio_fails is not None:
        _hit(counts, "single_candidate", int(best2 == 256))
        _hit(counts, "ratio_equality", int(bool(ratio_equal)))
        _hit(counts, "ratio_reject", int(bool(ratio_fails)))


def _count_bruteforce_query(counts, d, taken):
    free = np.nonzero(~taken)[0]
    if not len(free):
        _hit(counts, "no_train_left")
        return
    _hit(counts, "tie_at_best", int((d[free] == d[free].min()).sum() > 1))
    first = np.argsort(d, kind="stable")[:8]                  # the eight smallest (distance, index) keys
    _hit(counts, "blocked_by_call", int(taken[first[0]]))
    if d[first[0]] <= TH_LOW and len(d) > 8 and int((~taken[first]).sum()) < 2:
        _hit(counts, "rescan")


class Grid:
    """mGrid[ix][iy] of a frame: PosInGrid on every keypoint in order (a keypoint outside the grid is in no cell)"""

    def __init__(self, x, y, grid):
        self.x, self.y = np.asarray(x, F32), np.asarray(y, F32)
        self.min_x, self.min_y, self.gw_inv, self.gh_inv = [F32(v) for v in grid]
        self.cells = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
        for i in range(len(self.x)):
            px = _c_round(F32(F32(self.x[i] - self.min_x) * self.gw_inv))
            py = _c_round(F32(F32(self.y[i] - self.min_y) * self.gh_inv))
            if px < 0 or px >= GRID_COLS or py < 0 or py >= GRID_ROWS:
                continue
            self.cells[px][py].append(i)

    def features_in_area(self, x, y, r, octave, min_level=-1, max_level=-1, counts=None):
        """counts: "window_over_16_columns" (the device walks a window 16 grid columns at a time) and "level_skip", the features
        inside the window that the level range drops"""
        x, y, r = F32(x), F32(y), F32(r)
        out = []
        c0 = max(0, int(math.floor(F32(F32(F32(x - self.min_x) - r) * self.gw_inv))))
        if c0 >= GRID_COLS:
            return out
        c1 = min(GRID_COLS - 1, int(math.ceil(F32(F32(F32(x - self.min_x) + r) * self.gw_inv))))
        if c1 < 0:
            return out
        r0 = max(0, int(math.floor(F32(F32(F32(y - self.min_y) - r) * self.gh_inv))))
        if r0 >= GRID_ROWS:
            return out
        r1 = min(GRID_ROWS - 1, int(math.ceil(F32(F32(F32(y - self.min_y) + r) * self.gh_inv))))
        if r1 < 0:
            return out
        check = min_level > 0 or max_level >= 0
        _hit(counts, "window_over_16_columns", int(c1 - c0 + 1 > 16))
        for ix in range(c0, c1 + 1):
            for iy in range(r0, r1 + 1):
                for j in self.cells[ix][iy]:
                    if check:
                        if octave[j] < min_level or (max_level >= 0 and octave[j] > max_level):
                            if counts is not None:
                                _hit(counts, "level_skip", int(abs(F32(self.x[j] - x)) < r and abs(F32(self.y[j] - y)) < r))
                        if octave[j] < min_level:
                            continue
                        if max_level >= 0 and octave[j] > max_level:
                            continue
                    if abs(F32(self.x[j] - x)) < r and abs(F32(self.y[j] - y)) < r:
                        out.append(j)
        return out


def _mat3_vec_plus(T, v, accumulate):
    """rows 0..2 of the float 4 x 4 pose T: R v + t as the cv::Mat expression evaluates it (see the module text)"""
    out = []
    for r in range(3):
        if accumulate == "double":
            acc = float(T[r, 0]) * float(v[0]) + float(T[r, 1]) * float(v[1]) + float(T[r, 2]) * float(v[2])
            out.append(F32(F32(acc) + F32(T[r, 3])))
        else:
            acc = F32(F32(F32(T[r, 0]) * F32(v[0])) + F32(F32(T[r, 1]) * F32(v[1])))
            acc = F32(acc + F32(F32(T[r, 2]) * F32(v[2])))
            out.append(F32(acc + F32(T[r, 3])))
    return out


def frame_projection(tcw, K6, xw, accumulate="double"):
    """one world point through the frame-to-frame search's projection -> (invzc, u, v, uR), every step a float32"""
    fx, fy, cx, cy, mbf, _ = [F32(v) for v in K6]
    xc, yc, zc = _mat3_vec_plus(np.asarray(tcw, F32), xw, accumulate)
    invzc = F32(1.0 / float(zc))                           # const float invzc = 1.0 / x3Dc.at<float>(2): double division, float result
    u = F32(F32(F32(fx * xc) * invzc) + cx)
    v = F32(F32(F32(fy * yc) * invzc) + cy)
    return invzc, u, v, F32(u - F32(mbf * invzc))


def _count_window(counts, qd, tdesc, static, occupied, blocked, want):
    """static: the window's candidates after the filters that do not depend on the other queries, in traversal order (what the device
    stores: 256 per window in its everyday key format).  "scan_path": more than four of them free at entry, and fewer of the four
    best (distance, position) of those still unclaimed than the decision reads"""
    _hit(counts, "over_256_candidates", int(len(static) > 256))
    _hit(counts, "over_1024_candidates", int(len(static) > 1024))            # beyond the wide format: the device reports PS_ERR_CAPACITY
    free = [j for j in static if not occupied[j]]
    if len(free) > 4:
        four = np.argsort(_distances(qd, tdesc[free]), kind="stable")[:4]
        _hit(counts, "scan_path", int(sum(not blocked[free[k]] for k in four) < want))


def search_by_projection_frame(pr, check_ori=True, accumulate="double", counts=None):
    """-> (nmatches, match_of_train[n]): -1 untouched, -2 assigned in this call and set to NULL again by the rotation check.
    counts (a dict) receives how often each gate was passed."""
    T, q = pr["train"], pr["query"]
    n = len(T["x"])
    g = Grid(T["x"], T["y"], T["grid"])
    toct, tang, tur, tdesc = np.asarray(T["octave"]), np.asarray(T["angle"], F32), np.asarray(T["u_right"], F32), np.asarray(T["desc"], np.uint8).reshape(-1, 32)
    occupied = np.asarray(T["occupied"]).astype(bool)
    blocked = occupied.copy()
    tcw, tlw = np.asarray(pr["tcw"], F32), np.asarray(pr["tlw"], F32)
    fx, fy, cx, cy, mbf, mb = [F32(v) for v in pr["K6"]]
    minx, maxx, miny, maxy = [F32(v) for v in pr["bounds"]]
    sf = np.asarray(pr["scale_factors"], F32)
    th = F32(pr["th"])
    mono = bool(pr.get("mono"))
    # twc = -Rcw.t() * tcw, tlc = Rlw * twc + tlw  (only the sign and size of tlc[2] against the baseline are used)
    Rcw, t = tcw[:3, :3].astype(np.float64), tcw[:3, 3].astype(np.float64)
    twc = (-(Rcw.T @ t)).astype(F32)                       # (a transposed operand: gemm's general path, double accumulators)
    tlc2 = _mat3_vec_plus(tlw, twc, accumulate)[2]
    forward = bool(tlc2 > mb) and not mono
    backward = bool(-tlc2 > mb) and not mono
    _hit(counts, "mono" if mono else "forward" if forward else "backward" if backward else "neither")
    out = np.full(n, -1, np.int64)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nm = 0
    qxw, qvalid, qoct, qang = np.asarray(q["xw"], F32), np.asarray(q["valid"]), np.asarray(q["octave"]), np.asarray(q["angle"], F32)
    qdesc, qobs = np.asarray(q["desc"], np.uint8).reshape(-1, 32), np.asarray(q["observed"])
    for i in range(len(qvalid)):
        if not qvalid[i]:
            _hit(counts, "invalid")
            continue
        invzc, u, v, ur = frame_projection(tcw, pr["K6"], qxw[i], accumulate)
        if invzc < 0:
            _hit(counts, "behind_camera")
            continue
        if u < minx or u > maxx or v < miny or v > maxy:
            _hit(counts, "out_of_bounds")
            continue
        lo = int(qoct[i])
        radius = F32(th * sf[lo])
        if forward:
            cand = g.features_in_area(u, v, radius, toct, lo, -1, counts)
        elif backward:
            cand = g.features_in_area(u, v, radius, toct, 0, lo, counts)
        else:
            cand = g.features_in_area(u, v, radius, toct, lo - 1, lo + 1, counts)
        if not cand:
            _hit(counts, "empty_window")
            continue
        if counts is not None:
            _count_window(counts, qdesc[i], tdesc, [j for j in cand if not (tur[j] > 0 and abs(F32(ur - tur[j])) > radius)], occupied, blocked, 1)
        best, bidx, nbest = 256, -1, 0
        for j in cand:
            if blocked[j]:
                _hit(counts, "blocked_at_entry" if occupied[j] else "blocked_by_call")
                continue
            if tur[j] > 0:
                if abs(F32(ur - tur[j])) > radius:
                    _hit(counts, "ur_gate")
                    continue
            d = descriptor_distance(qdesc[i], tdesc[j])
            nbest = 1 if d < best else nbest + (d == best)
            if d < best:
                best, bidx = d, j
        if counts is not None:
            _hit(counts, "all_filtered", int(bidx < 0))
            _hit(counts, "tie_at_best", int(nbest > 1))
            if bidx >= 0:
                _count_decision(counts, best, 256, TH_HIGH, None, None)
        if best <= TH_HIGH:
            _hit(counts, "accepted")
            _hit(counts, "overwrite_unobserved", int(out[bidx] != -1))
            out[bidx] = i
            if qobs[i]:
                blocked[bidx] = True
            nm += 1
            if check_ori:
                hist[_rot_bin(qang[i], tang[bidx], counts)].append(bidx)
    if check_ori:
        nm -= _rotation_check(hist, out, -2, counts)
    return nm, out.astype(np.int32)


def search_by_projection_points(pr, nnratio, obj=False, counts=None):
    """the local-map overload (obj=False) and the object overload (obj=True: fixed 5-pixel window, levels -1 .. +1, bounding-box test,
    threshold 130) -> (nmatches, match_of_train[n]).  counts (a dict) receives how often each gate was passed."""
    T, q = pr["train"], pr["query"]
    n = len(T["x"])
    g = Grid(T["x"], T["y"], T["grid"])
    toct, tur, tdesc = np.asarray(T["octave"]), np.asarray(T["u_right"], F32), np.asarray(T["desc"], np.uint8).reshape(-1, 32)
    inbox = np.asarray(T.get("in_bbox", np.ones(n, np.uint8)))
    occupied = np.asarray(T["occupied"]).astype(bool)
    blocked = occupied.copy()
    sf = np.asarray(pr["scale_factors"], F32)
    th = F32(pr["th"])
    factor = bool(th != F32(1.0))
    out = np.full(n, -1, np.int64)
    nm = 0
    valid, px, py, pxr = np.asarray(q["valid"]), np.asarray(q["proj_x"], F32), np.asarray(q["proj_y"], F32), np.asarray(q["proj_xr"], F32)
    lvl, vc, qdesc, qobs = np.asarray(q["level"]), np.asarray(q["view_cos"], F32), np.asarray(q["desc"], np.uint8).reshape(-1, 32), np.asarray(q["observed"])
    limit = TH_HIGH_FORDYNAMIC if obj else TH_HIGH
    for i in range(len(valid)):
        if not valid[i]:
            _hit(counts, "invalid")
            continue
        level = int(lvl[i])
        r = F32(2.5) if float(vc[i]) > 0.998 else F32(4.0)          # the comparison promotes the float to double
        if factor:
            r = F32(r * th)
        if obj:
            cand = g.features_in_area(px[i], py[i], F32(5), toct, level - 1, level + 1, counts)
        else:
            cand = g.features_in_area(px[i], py[i], F32(r * sf[level]), toct, level - 1, level, counts)
        if not cand:
            _hit(counts, "empty_window")
            continue
        if counts is not None:
            static = [j for j in cand if not (obj and not inbox[j]) and not (tur[j] > 0 and abs(F32(pxr[i] - tur[j])) > F32(r * sf[level]))]
            _count_window(counts, qdesc[i], tdesc, static, occupied, blocked, 2)
        best, best2, blevel, blevel2, bidx, nbest = 256, 256, -1, -1, -1, 0
        for j in cand:
            if obj and not inbox[j]:
                _hit(counts, "bbox_skip")
                continue
            if blocked[j]:
                _hit(counts, "blocked_at_entry" if occupied[j] else "blocked_by_call")
                continue
            if tur[j] > 0:
                if abs(F32(pxr[i] - tur[j])) > F32(r * sf[level]):
                    _hit(counts, "ur_gate")
                    continue
            d = descriptor_distance(qdesc[i], tdesc[j])
            nbest = 1 if d < best else nbest + (d == best)
            if d < best:
                best2, best, blevel2, blevel, bidx = best, d, blevel, int(toct[j]), j
            elif d < best2:
                blevel2, best2 = int(toct[j]), d
        if counts is not None:
            _hit(counts, "all_filtered", int(bidx < 0))
            _hit(counts, "tie_at_best", int(nbest > 1))
            if bidx >= 0:
                over, equal = F32(best) > F32(nnratio) * F32(best2), F32(best) == F32(nnratio) * F32(best2)
                _count_decision(counts, best, best2, limit, over and blevel == blevel2, None)
                if best <= limit and best2 < 256:
                    _hit(counts, "ratio_equality_same_level" if blevel == blevel2 else "ratio_equality_other_level", int(bool(equal)))
                    _hit(counts, "ratio_saved_by_level", int(bool(over) and blevel != blevel2))
        if best <= limit:
            if blevel == blevel2 and F32(best) > F32(nnratio) * F32(best2):
                continue
            _hit(counts, "accepted")
            _hit(counts, "overwrite_unobserved", int(out[bidx] != -1))
            out[bidx] = i
            if qobs[i]:
                blocked[bidx] = True
            nm += 1
    return nm, out.astype(np.int32)


# ---- the search half of ORBmatcher::Fuse(ObjectKeyFrame*, points, th)   /root/reference/src/ORBmatcher.cc:1138-1260 -----------------------------
def fuse_geometry(pr, i, accumulate="double", counts=None):
    """candidate point i up to its search window: None when a gate drops it, else (u, v, ur, level, radius).  Every float of the
    reference a numpy float32; `Rco * Poj + tco` by either reading of the cv::Mat expression (the module text); cv::norm and Mat::dot
    accumulate in double; GetMin / MaxDistanceInvariance apply 0.8f / 1.2f."""
    q = pr["query"]
    fx, fy, cx, cy, bf = [F32(v) for v in pr["K5"]]
    R, t, ow = np.asarray(pr["R"], F32), np.asarray(pr["t"], F32), np.asarray(pr["ow"], F32)
    Tm = np.zeros((3, 4), F32); Tm[:, :3] = R; Tm[:, 3] = t
    b = [float(v) for v in pr["bounds"]]
    sf = np.asarray(pr["scale_factors"], F32)
    logsf, nlev, th = F32(pr["log_scale_factor"]), int(pr["n_levels"]), F32(pr["th"])
    P = np.asarray(q["pos"][i], F32)
    pc = _mat3_vec_plus(Tm, P, accumulate)
    if pc[2] < 0:
        _hit(counts, "behind_camera")
        return None
    invz = F32(F32(1) / pc[2])
    x, y = F32(pc[0] * invz), F32(pc[1] * invz)
    u, v = F32(F32(fx * x) + cx), F32(F32(fy * y) + cy)
    ur = F32(u - F32(bf * invz))
    if not (float(u) >= b[0] and float(u) < b[1] and float(v) >= b[2] and float(v) < b[3]):
        _hit(counts, "outside_bounds")
        return None
    po = [F32(P[c] - ow[c]) for c in range(3)]
    dist = F32(math.sqrt(sum(float(c) * float(c) for c in po)))
    if dist < F32(F32(0.8) * F32(q["min_dist"][i])) or dist > F32(F32(1.2) * F32(q["max_dist"][i])):
        _hit(counts, "outside_distance_range")
        return None
    n = np.asarray(q["normal"][i], F32)
    if sum(float(po[c]) * float(n[c]) for c in range(3)) < 0.5 * float(dist):
        _hit(counts, "view_angle")
        return None
    ratio = F32(F32(q["max_dist"][i]) / dist)
    lvl = int(math.ceil(math.log(float(ratio)) / float(logsf)))
    _hit(counts, "level_clamped_low", int(lvl < 0))
    _hit(counts, "level_clamped_high", int(lvl > nlev - 1))
    lvl = 0 if lvl < 0 else min(lvl, nlev - 1)
    return u, v, ur, lvl, F32(th * sf[lvl])


def fuse_search(pr, accumulate="double", counts=None):
    """-> (best_idx, best_dist) per candidate point.  counts (a dict) receives how often each gate was passed."""
    T, q = pr["train"], pr["query"]
    g = Grid(T["x"], T["y"], T["grid"])
    tx, ty, toct, tur, tdesc = np.asarray(T["x"], F32), np.asarray(T["y"], F32), np.asarray(T["octave"]), np.asarray(T["u_right"], F32), np.asarray(T["desc"], np.uint8).reshape(-1, 32)
    is2 = np.asarray(pr["inv_level_sigma2"], F32)
    m = len(q["valid"])
    bi, bd = np.full(m, -1, np.int32), np.full(m, 256, np.int32)
    for i in range(m):
        if not q["valid"][i]:
            _hit(counts, "invalid")
            continue
        geo = fuse_geometry(pr, i, accumulate, counts)
        if geo is None:
            continue
        u, v, ur, lvl, radius = geo
        best, bidx, nbest = 256, -1, 0
        cand = g.features_in_area(u, v, radius, toct, counts=counts)
        _hit(counts, "empty_window", int(not cand))
        for j in cand:
            kl = int(toct[j])
            if kl < lvl - 1 or kl > lvl:
                _hit(counts, "level_skip")
                continue
            ex, ey = F32(u - tx[j]), F32(v - ty[j])
            if tur[j] >= 0:
                er = F32(ur - tur[j])
                e2 = F32(F32(F32(ex * ex) + F32(ey * ey)) + F32(er * er))
                if float(F32(e2 * is2[kl])) > 7.8:
                    _hit(counts, "chi2_stereo")
                    continue
            else:
                e2 = F32(F32(ex * ex) + F32(ey * ey))
                if float(F32(e2 * is2[kl])) > 5.99:
                    _hit(counts, "chi2_mono")
                    continue
            d = descriptor_distance(np.asarray(q["desc"][i], np.uint8), tdesc[j])
            nbest = 1 if d < best else nbest + (d == best)
            if d < best:
                best, bidx = d, j
        bd[i] = best
        if counts is not None and bidx >= 0:
            _hit(counts, "tie_at_best", int(nbest > 1))
            _hit(counts, "best_eq_50", int(best == 50))
            _hit(counts, "best_eq_51", int(best == 51))
        if best <= 50:
            _hit(counts, "accepted")
            bi[i] = bidx
    return bi, bd
