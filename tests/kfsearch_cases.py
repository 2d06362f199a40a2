"""The seeded cases of tests/test_kfsearch_gpu.py, built once and shared with tests/test_kfsearch_cpu.py, which checks on the CPU
that every one of them covers what it is named for and meets the input condition of the GPU comparison (no predicted level within
4 ulp of a boundary).  The problems are the dicts ORBmatcher.KfSearch / SearchBySim3 take; the answers come from
tests/kfsearch_second_opinion.py.  Camera as in tests/test_tri_cpu.py, 1241 x 376 bounds, 8 levels at 1.2.  Test infrastructure."""
import copy
import functools
import math

import numpy as np

from pointslot_amd import matcher
import kfsearch_second_opinion as so

F32 = np.float32
FX, FY, CX, CY = 700.0, 700.0, 600.0, 180.0
W, H = 1241.0, 376.0
BOUNDS = (0.0, W, 0.0, H)
GRID = (F32(0.0), F32(0.0), F32(64.0) / F32(W), F32(48.0) / F32(H))
SF = np.array([1.2 ** l for l in range(8)], F32)
LOGS = F32(math.log(1.2))
V_FREE = 60.0          # no feature of a generated scene lies above this image row: the "empty" windows are up there


def _rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def _flip(rng, d, k):
    d = d.copy()
    for b in rng.choice(256, k, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _flip_bits(d, bits):
    d = d.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _scw_pose(rng, s=1.0, rot=0.05, trans=0.5):
    """(R, t, ow) float32 the way the caller of the Sim3 overloads gets them: a Sim3 matrix through decompose_scw"""
    R, t = _rot(rng.normal(0, rot, 3)), rng.normal(0, trans, 3)
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = s * R, s * t
    Rcw, tcw, ow, _ = matcher.decompose_scw(S.astype(F32))
    return Rcw, tcw, ow


def _frame_pose(rng, rot=0.05, trans=0.5):
    """(R, t, ow) of a Frame's mTcw: Ow = -Rcw^T tcw, products and sum in double, rounded once"""
    R, t = _rot(rng.normal(0, rot, 3)).astype(F32), rng.normal(0, trans, 3).astype(F32)
    ow = np.array([F32(-(float(R[0, r]) * float(t[0]) + float(R[1, r]) * float(t[1]) + float(R[2, r]) * float(t[2]))) for r in range(3)], F32)
    return R, t, ow


def _world(R, t, xc):
    return (R.astype(np.float64).T @ (np.asarray(xc, np.float64) - t.astype(np.float64))).astype(F32)


def _cam_of_pixel(u, v, z):
    return np.array([(u - CX) * z / FX, (v - CY) * z / FY, z])


class _Scene:
    """features of the searched side and the points projected into it, appended one by one"""

    def __init__(self, rng, mode, pose):
        self.rng, self.mode = rng, mode
        self.R, self.t, self.ow = pose
        self.f, self.q = [], []

    def feature(self, u, v, octave, desc, angle=0.0, occupied=0):
        self.f.append((u, v, octave, angle, occupied, desc))
        return len(self.f) - 1

    def point(self, xc, desc, level, valid=1, angle=0.0, normal_sign=1.0, max_scale=1.0, frac=None):
        """a map point at camera-frame position xc whose PredictScale gives `level` (max_scale = 1)"""
        xw = _world(self.R, self.t, xc)
        po = xw.astype(np.float64) - self.ow.astype(np.float64)
        dist = np.linalg.norm(po)
        frac = self.rng.uniform(-0.8, -0.2) if frac is None else frac
        maxd = dist * 1.2 ** (level + frac) * max_scale
        nrm = po / dist + self.rng.normal(0, 0.05, 3)
        nrm = normal_sign * nrm / np.linalg.norm(nrm)
        self.q.append((valid, xw, nrm.astype(F32), F32(maxd / 1.2 ** 7), F32(maxd), desc, angle))
        return len(self.q) - 1

    def problem(self, th, **kw):
        f, q = self.f, self.q
        col = lambda rows, i, dt: np.array([r[i] for r in rows], dt)
        x, y = col(f, 0, F32), col(f, 1, F32)
        cell_off, cell_idx = matcher.build_grid(x, y, *GRID)
        train = dict(x=x, y=y, octave=col(f, 2, np.int32), angle=col(f, 3, F32), occupied=col(f, 4, np.uint8),
                     desc=np.array([r[5] for r in f], np.uint8).reshape(-1, 32), cell_off=cell_off, cell_idx=cell_idx, grid=GRID)
        query = dict(valid=col(q, 0, np.uint8), pos=np.array([r[1] for r in q], F32).reshape(-1, 3),
                     normal=np.array([r[2] for r in q], F32).reshape(-1, 3), min_dist=col(q, 3, F32), max_dist=col(q, 4, F32),
                     desc=np.array([r[5] for r in q], np.uint8).reshape(-1, 32), angle=col(q, 6, F32))
        pr = dict(mode=self.mode, train=train, query=query, R=self.R, t=self.t, ow=self.ow, K4=(F32(FX), F32(FY), F32(CX), F32(CY)),
                  bounds=BOUNDS, scale_factors=SF, log_scale_factor=LOGS, n_levels=8, th=F32(th))
        pr.update(kw)
        return pr


def _new_desc(rng):
    return rng.randint(0, 256, 32).astype(np.uint8)


def _pose_for(rng, mode):
    return _frame_pose(rng) if mode == 2 else _scw_pose(rng, s=rng.choice([1.0, 0.93, 1.07]))


def _angle_pair(rng, spread):
    """(query angle, train angle) in [0, 360) with the difference drawn from a mixture (spread: uniform over the circle)"""
    ta = rng.uniform(0, 360)
    if spread:
        rot = rng.uniform(0, 360)
    else:
        r = rng.rand()
        rot = rng.uniform(0, 25) if r < 0.7 else (rng.uniform(80, 100) if r < 0.9 else rng.uniform(0, 360))
    return F32((ta + rot) % 360.0), F32(ta)


def _main(mode, seed, nf=500, nq=500, th=10.0, spread=False, first=0, **kw):
    """first: where in the cycle of 29 point kinds the case starts (7: behind the special ones, so a short case has plain points)"""
    rng = np.random.RandomState(seed)
    sc = _Scene(rng, mode, _pose_for(rng, mode))
    n_seen = min(nf, nq) * 7 // 10
    special = ["invalid", "depth", "image", "distance", "empty", "nomatch"] + ([] if mode == 2 else ["angle"])
    for i in range(nq):
        u, v, z = rng.uniform(30, W - 30), rng.uniform(V_FREE + 10, H - 20), rng.uniform(4, 40)
        xc = _cam_of_pixel(u, v, z)
        qa, ta = _angle_pair(rng, spread)
        octave = int(rng.randint(0, 8))
        desc = _new_desc(rng)
        if i < n_seen:
            sc.feature(u + rng.uniform(-1.5, 1.5), v + rng.uniform(-1.5, 1.5), octave, desc, angle=ta, occupied=int(rng.rand() < 0.1))
        # the predicted level against the feature's octave: inside the member's window, at its edges, and one step outside
        level = int(np.clip(octave + rng.choice([0, 0, 1, 1, -1, 2]), 0, 7))
        kind = special[(i + first) % 29] if (i + first) % 29 < len(special) else "plain"
        pd = _flip(rng, desc, int(rng.randint(0, 61)))
        if kind == "invalid":
            sc.point(xc, pd, level, valid=0, angle=qa)
        elif kind == "depth":          # behind the camera, on the same ray: the same pixel
            sc.point(-xc, pd, level, angle=qa, normal_sign=1.0)
        elif kind == "image":
            sc.point(_cam_of_pixel(W + rng.uniform(5, 80), v, z), pd, level, angle=qa)
        elif kind == "distance":
            sc.point(xc, pd, level, angle=qa, max_scale=rng.choice([0.3, 40.0]))
        elif kind == "angle":
            sc.point(xc, pd, level, angle=qa, normal_sign=-1.0)
        elif kind == "empty":
            sc.point(_cam_of_pixel(u, rng.uniform(5, 20), z), pd, 0, angle=qa)
        elif kind == "nomatch":
            sc.point(xc, _new_desc(rng), level, angle=qa)
        else:
            sc.point(xc, pd, level, angle=qa)
    while len(sc.f) < nf:              # features nothing was projected from; some sit beside a seen one with a similar descriptor
        if sc.f and rng.rand() < 0.4:
            u0, v0, o0, a0, _, d0 = sc.f[rng.randint(len(sc.f))]
            sc.feature(float(np.clip(u0 + rng.uniform(-6, 6), 1, W - 2)), float(np.clip(v0 + rng.uniform(-6, 6), V_FREE, H - 2)), o0,
                       _flip(rng, d0, int(rng.randint(5, 70))), angle=a0, occupied=int(rng.rand() < 0.1))
        else:
            sc.feature(rng.uniform(1, W - 2), rng.uniform(V_FREE, H - 2), int(rng.randint(0, 8)), _new_desc(rng), angle=rng.uniform(0, 360))
    return sc.problem(th, **kw)


def _contention(mode):
    """Three points want slot F0, which P0 gets; P1's next candidate F1 is under the threshold, P2's next one F2 as well; Q0 gets G0 and
    Q1's next candidate G1 is over the threshold; FOCC would be everybody's best and is occupied at entry."""
    rng = np.random.RandomState(40 + mode)
    sc = _Scene(rng, mode, _pose_for(rng, mode))
    th_dist = 64 if mode == 2 else 50
    D, E = _new_desc(rng), _new_desc(rng)
    xa, xb = _cam_of_pixel(400.0, 200.0, 10.0), _cam_of_pixel(900.0, 250.0, 12.0)
    focc = sc.feature(400.5, 200.5, 2, D, occupied=1)
    f0 = sc.feature(401.0, 199.0, 2, D)
    f1 = sc.feature(399.0, 201.0, 2, _flip_bits(D, range(100, 120)))
    f2 = sc.feature(402.0, 202.0, 2, _flip_bits(D, range(100, 145)))
    g0 = sc.feature(900.5, 250.5, 3, E)
    g1 = sc.feature(899.0, 249.0, 3, _flip_bits(E, range(100, 100 + th_dist + 6)))
    for k in range(20):
        sc.feature(rng.uniform(1, W - 2), rng.uniform(V_FREE, 150), int(rng.randint(0, 8)), _new_desc(rng))
    p0 = sc.point(xa, _flip_bits(D, [0, 1]), 2)
    p1 = sc.point(xa, _flip_bits(D, [2, 3, 4]), 2)
    p2 = sc.point(xa, _flip_bits(D, [5, 6, 7, 8]), 2)
    p3 = sc.point(xa, _flip_bits(D, [9]), 2)                   # everything it could take is gone
    q0 = sc.point(xb, _flip_bits(E, [0]), 3)
    q1 = sc.point(xb, _flip_bits(E, [1, 2]), 3)
    pr = sc.problem(10.0, th_dist=th_dist, check_orientation=1)
    pr["expect"] = {focc: -1, f0: p0, f1: p1, f2: p2, g0: q0, g1: -1}
    pr["expect_unmatched"] = [p3, q1]
    return pr


def _tie(mode):
    """two features with the same descriptor left and right of the projection, the LEFT one (earlier grid column, first in traversal
    order) at the HIGHER index: the first strict minimum is the left one"""
    rng = np.random.RandomState(50 + mode)
    sc = _Scene(rng, mode, _pose_for(rng, mode))
    pairs = []
    for k in range(6):
        u, v = 150.0 + 180.0 * k, 120.0 + 30.0 * k
        d = _new_desc(rng)
        right = sc.feature(u + 12.0, v, 3, d)
        for _ in range(3):
            sc.feature(rng.uniform(1, W - 2), rng.uniform(300, H - 2), 0, _new_desc(rng))
        left = sc.feature(u - 12.0, v, 3, d)
        p = sc.point(_cam_of_pixel(u, v, 9.0 + k), _flip(rng, d, 5), 3)
        pairs.append((p, left, right))
    pr = sc.problem(10.0, check_orientation=0)
    pr["expect_tie"] = pairs
    return pr


def _behind(mode):
    """a point behind the camera whose projection is in bounds, with its feature: searched by mode 2, rejected by mode 0"""
    rng = np.random.RandomState(60)
    sc = _Scene(rng, mode, _frame_pose(rng))
    d = _new_desc(rng)
    f = sc.feature(500.0, 200.0, 1, d)
    p = sc.point(-_cam_of_pixel(500.0, 200.0, 7.0), _flip(rng, d, 3), 1)
    pr = sc.problem(10.0, check_orientation=0)
    pr["expect_behind"] = (p, f)
    return pr


def _edge(mode):
    """u exactly mnMaxX: inside the inclusive bounds of mode 2, outside the exclusive ones of modes 0 / 1"""
    rng = np.random.RandomState(61)
    xp = F32(641.0 / 700.0)
    for _ in range(64):                       # a float x' with float(700 * x') == 641 exactly; z = 8 keeps every other step exact
        got = F32(F32(FX) * xp)
        if got == F32(641.0):
            break
        xp = np.nextafter(xp, F32(2.0) if got < F32(641.0) else F32(0.0))
    assert F32(F32(FX) * xp) == F32(641.0)
    I = np.eye(3, dtype=F32)
    z = np.zeros(3, F32)
    sc = _Scene(rng, mode, (I, z, z))
    d = _new_desc(rng)
    f = sc.feature(1228.0, 180.0, 2, d)      # (a keypoint right of 1231.3 rounds to grid column 64: in no cell)
    p = sc.point(np.array([float(xp) * 8.0, 0.0, 8.0]), _flip(rng, d, 4), 2)
    pr = sc.problem(10.0, check_orientation=0)
    pr["expect_edge"] = (p, f)
    return pr


def _wide(mode):
    """300 features inside one 30-pixel window, all within the threshold of the points projected there: more candidates a point
    could take than the everyday store keeps - the wide re-run"""
    rng = np.random.RandomState(70 + mode)
    sc = _Scene(rng, mode, _pose_for(rng, mode))
    d = _new_desc(rng)
    for k in range(300):
        sc.feature(600.0 + rng.uniform(-15, 15), 200.0 + rng.uniform(-15, 15), 4, _flip(rng, d, int(rng.randint(2, 40))), occupied=int(k % 50 == 0))
    for k in range(40):
        sc.feature(rng.uniform(1, W - 2), rng.uniform(300, H - 2), 0, _new_desc(rng))
    for k in range(12):
        sc.point(_cam_of_pixel(600.0 + rng.uniform(-2, 2), 200.0 + rng.uniform(-2, 2), 10.0), _flip(rng, d, int(rng.randint(0, 6))), 4)
    return sc.problem(10.0, th_dist=64, check_orientation=0)


def _reordered(pr, order):
    """the searched side's features in another order: new feature j is old feature order[j] (pr is changed in place and returned)"""
    t = pr["train"]
    for k in ("x", "y", "octave", "angle", "occupied", "desc"):
        t[k] = np.ascontiguousarray(t[k][order])
    t["cell_off"], t["cell_idx"] = matcher.build_grid(t["x"], t["y"], *GRID)
    return pr


def _limit(mode, seed, **kw):
    """8191 searched features, the documented limit, and 3000 points; the features in a random order, so that the matches (_main puts
    the features it projects from first) fall on both sides of index 4096: every bit of the candidate key's 13-bit index and every word
    of ks_resolve's 8192-bit bitmap"""
    pr = _main(mode, seed, nf=8191, nq=3000, **kw)
    return _reordered(pr, np.random.RandomState(seed + 1).permutation(8191))


def _over():
    """three problems, the second with 8192 features: it alone fails"""
    big = _main(0, 81, nf=8192, nq=20)
    return [_main(0, 80, nf=120, nq=90), big, _main(2, 82, nf=120, nq=90)]


def _empty(mode, which, **kw):
    pr = _main(mode, 90 + mode, nf=60, nq=40) if not kw else _main(mode, **kw)
    if which == "nq":
        pr["query"] = {k: v[:0] for k, v in pr["query"].items()}
    else:
        t = pr["train"]
        for k in ("x", "y", "octave", "angle", "occupied", "desc"):
            t[k] = t[k][:0]
        t["cell_off"], t["cell_idx"] = matcher.build_grid(t["x"], t["y"], *GRID)
    return pr


# ---- SearchBySim3 ----------------------------------------------------------------------------------------------------------
def _sim3(seed, s12=1.0, n=500, tie=False):
    """Two keyframes 1 - 3 m apart that see the same physical points; keyframe 2's map is drifted in scale by 1 / s12, which the
    Sim3 (s12, R12, t12) undoes.  Two thirds of the slots carry points; some pairs agree, some match one way only."""
    rng = np.random.RandomState(seed)
    R1, t1 = _rot(rng.normal(0, 0.03, 3)).astype(F32), rng.normal(0, 0.3, 3).astype(F32)
    R2 = (_rot(rng.normal(0, 0.03, 3)) @ R1.astype(np.float64)).astype(F32)
    t2 = (t1.astype(np.float64) + np.array([rng.uniform(1.0, 3.0) * rng.choice([-1, 1]), rng.normal(0, 0.1), rng.normal(0, 0.3)])).astype(F32)
    # true relative motion c1 = R12 c2 + t12 (scale 1), then the drift
    R12 = R1.astype(np.float64) @ R2.astype(np.float64).T
    t12 = t1.astype(np.float64) - R12 @ t2.astype(np.float64)
    sr12, t12f, sr21, t21 = matcher.sim3_pair(s12, R12, t12)
    f1, f2 = [], []                           # (u, v, octave, desc)
    slots1, slots2 = {}, {}                   # slot -> dict(pos, max, desc)
    expect_tie = []

    def pt(c_other_dist, level, desc, pos):
        maxd = c_other_dist * 1.2 ** (level + rng.uniform(-0.8, -0.2))
        return dict(pos=pos, max=F32(maxd), desc=desc)

    while len(f1) < n or len(f2) < n:
        u2, v2, z2 = rng.uniform(40, W - 40), rng.uniform(V_FREE + 10, H - 20), rng.uniform(5, 40)
        c2 = _cam_of_pixel(u2, v2, z2)                      # cam 2, true scale
        c1 = R12 @ c2 + t12
        u1, v1 = FX * c1[0] / c1[2] + CX, FY * c1[1] / c1[2] + CY
        o1, o2 = int(rng.randint(0, 8)), int(rng.randint(0, 8))
        d1, d2 = _new_desc(rng), _new_desc(rng)
        vis1 = c1[2] > 1 and 20 < u1 < W - 20 and V_FREE < v1 < H - 10
        r = rng.rand()
        i1 = i2 = None
        if len(f1) < n and vis1:
            f1.append((u1 + rng.uniform(-1, 1), v1 + rng.uniform(-1, 1), o1, d1)); i1 = len(f1) - 1
        if len(f2) < n:
            f2.append((u2 + rng.uniform(-1, 1), v2 + rng.uniform(-1, 1), o2, d2)); i2 = len(f2) - 1
        c2m = c2 / s12                                      # cam 2 in keyframe 2's drifted map
        xw1, xw2 = _world(R1, t1, c1), _world(R2, t2, c2m)
        # the point of slot i1 is searched in keyframe 2 (distance |c2m|, features of octave o2), and the other way round
        plain1 = plain2 = False
        if i1 is not None and r < 0.67:
            slots1[i1] = pt(np.linalg.norm(c2m), min(7, o2 + int(rng.randint(0, 2))), _flip(rng, d2, int(rng.randint(0, 61))) if r < 0.6 else _new_desc(rng), xw1)
            sp = rng.rand()
            if sp < 0.03:                                   # behind keyframe 2
                slots1[i1]["pos"] = _world(R1, t1, R12 @ (-c2) + t12)
            elif sp < 0.06:                                 # outside the scale-invariance region
                slots1[i1]["max"] = F32(slots1[i1]["max"] * rng.choice([0.3, 40.0]))
            plain1 = r < 0.6 and sp >= 0.06
        if i2 is not None and (r < 0.45 or 0.67 <= r < 0.85):
            one_way = i1 is None or rng.rand() < 0.15
            slots2[i2] = pt(np.linalg.norm(c1), min(7, o1 + int(rng.randint(0, 2))), _new_desc(rng) if one_way else _flip(rng, d1, int(rng.randint(0, 61))), xw2)
            plain2 = not one_way
        if tie and plain1 and plain2 and o2 >= 4 and len(expect_tie) < 5 and len(f2) + 1 < n and 60 < u2 < W - 60:
            # the partner in keyframe 2 becomes the RIGHT one of an equal pair (window half-size >= 7.5 * 1.2^4 > 12); its copy on the
            # left gets the higher index ...
            f2[i2] = (u2 + 12.0, v2, o2, d2)
            f2.append((u2 - 12.0, v2, o2, d2))
            slots2[len(f2) - 1] = slots2.pop(i2)            # ... and the point, so that the two directions can agree on it
            expect_tie.append((i1, len(f2) - 1, i2))

    def side(f, slots, R, t, fx):
        nn = len(f)
        x, y = np.array([r_[0] for r_ in f], F32), np.array([r_[1] for r_ in f], F32)
        cell_off, cell_idx = matcher.build_grid(x, y, *GRID)
        has = np.zeros(nn, np.uint8); pos = np.zeros((nn, 3), F32); mx = np.ones(nn, F32); pd = np.zeros((nn, 32), np.uint8)
        for i, s_ in slots.items():
            has[i], pos[i], mx[i], pd[i] = 1, s_["pos"], s_["max"], s_["desc"]
        return dict(x=x, y=y, octave=np.array([r_[2] for r_ in f], np.int32), angle=np.zeros(nn, F32),
                    desc=np.array([r_[3] for r_ in f], np.uint8).reshape(-1, 32), cell_off=cell_off, cell_idx=cell_idx, grid=GRID,
                    has_point=has, pos=pos, min_dist=(mx / F32(1.2 ** 7)).astype(F32), max_dist=mx, point_desc=pd,
                    already=np.zeros(nn, np.uint8), R=R, t=t, bounds=BOUNDS, scale_factors=SF, log_scale_factor=LOGS, n_levels=8,
                    K4=(F32(fx), F32(FY), F32(CX), F32(CY)))

    kf1, kf2 = side(f1, slots1, R1, t1, FX), side(f2, slots2, R2, t2, 650.0)     # keyframe 2's own fx is never read
    pr = dict(kf1=kf1, kf2=kf2, K4=kf1["K4"], s12=F32(s12), R12=R12.astype(F32), t12=t12.astype(F32), th=F32(7.5))
    pr["expect_tie"] = expect_tie
    return pr


def _sim3_main(seed, s12):
    pr = _sim3(seed, s12)
    ref = so.search_by_sim3(pr)
    # 40 pairs that agree are handed in as matched already (vpMatches12 at entry)
    agreed = np.nonzero(ref["match12"] >= 0)[0][:40]
    m12 = np.full(len(pr["kf1"]["x"]), -1, np.int32)
    m12[agreed] = ref["match12"][agreed]
    pr["matches12"] = m12
    pr["kf1"]["already"] = (m12 >= 0).astype(np.uint8)
    a2 = np.zeros(len(pr["kf2"]["x"]), np.uint8)
    a2[m12[m12 >= 0]] = 1
    pr["kf2"]["already"] = a2
    return pr


KF_BUILDERS = {
    "main_0": lambda: _main(0, 11), "main_1": lambda: _main(1, 12, nf=600, nq=800, th=4.0), "main_2": lambda: _main(2, 13, nf=450, nq=450, th_dist=100),
    "main_2_64": lambda: _main(2, 14, nf=400, nq=300, th=3.0, th_dist=64),
    "contention_0": lambda: _contention(0), "contention_2": lambda: _contention(2),
    "tie_0": lambda: _tie(0), "tie_1": lambda: _tie(1), "tie_2": lambda: _tie(2),
    "behind_2": lambda: _behind(2), "behind_0": lambda: _behind(0),
    "edge_0": lambda: _edge(0), "edge_1": lambda: _edge(1), "edge_2": lambda: _edge(2),
    "rot13": lambda: _main(2, 15, nf=500, nq=500, spread=True, th_dist=100),
    "wide_0": lambda: _wide(0), "wide_2": lambda: _wide(2),
    "limit_0": lambda: _limit(0, 16), "limit_2": lambda: _limit(2, 17, th_dist=100),
    "empty_nq_0": lambda: _empty(0, "nq"), "empty_nq_1": lambda: _empty(1, "nq"), "empty_n_2": lambda: _empty(2, "n"), "empty_n_1": lambda: _empty(1, "n"),
}
KF_BUILDERS.update({"batch_%02d" % k: (lambda k=k: _main(k % 3, 100 + k, nf=90 + 17 * k, nq=70 + 13 * k, th=(10.0, 4.0, 10.0)[k % 3]))
                    for k in range(16)})
BATCH = tuple("batch_%02d" % k for k in range(16))
# one call, three problems, one of each mode: 65 features (one more than a wave) and 5 points each, the third searched side empty
KF_BUILDERS.update({"mixed_0": lambda: _main(0, 130, nf=65, nq=5, first=7), "mixed_1": lambda: _main(1, 131, nf=65, nq=5, th=4.0, first=7),
                    "mixed_2": lambda: _empty(2, "n", seed=132, nf=65, nq=5, first=7)})
MIXED = ("mixed_0", "mixed_1", "mixed_2")
SIM3_BUILDERS = {
    "sim3_main": lambda: _sim3_main(21, 1.0), "sim3_main_093": lambda: _sim3_main(22, 0.93),
    "sim3_tie": lambda: _sim3(23, 1.0, n=200, tie=True),
    "sim3_empty_1": lambda: _sim3_cut(24, 1), "sim3_empty_2": lambda: _sim3_cut(24, 2),
    "sim3_small": lambda: _sim3(25, 0.93, n=130),
}


def _sim3_cut(seed, which):
    pr = _sim3(seed, 1.0, n=80)
    kf = pr["kf%d" % which]
    for k in ("x", "y", "octave", "angle", "desc", "has_point", "pos", "min_dist", "max_dist", "point_desc", "already"):
        kf[k] = kf[k][:0]
    kf["cell_off"], kf["cell_idx"] = matcher.build_grid(kf["x"], kf["y"], *GRID)
    return pr


@functools.lru_cache(maxsize=None)
def _built(name):
    if name in KF_BUILDERS:
        pr = KF_BUILDERS[name]()
        return pr, so.run(pr)
    pr = SIM3_BUILDERS[name]()
    return pr, so.search_by_sim3(pr)


def problem(name):
    """a private copy of the case's problem dict (the arrays are shared: do not write into them)"""
    return copy.copy(_built(name)[0])


def reference(name):
    return _built(name)[1]


@functools.lru_cache(maxsize=None)
def over():
    return _over()
