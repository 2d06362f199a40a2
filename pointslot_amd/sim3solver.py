"""ORB_SLAM2::Sim3Solver over arrays: ps_sim3_ransac evaluates every hypothesis of every candidate keyframe pair in one device call, and
the reference's sequential loop (src/Sim3Solver.cc:141-208) becomes a cursor over the cached counts.

The draws: a solver takes its 3 x mRansacMaxIts raw rand() values when it is prepared (PrepareBatch, or its first iterate), not lazily
as the reference does, so the global rand() order across solvers differs from the reference's; the sample sets are i.i.d. either way."""
import ctypes

import numpy as np

from ._lib import lib, check
from .matcher import ORBmatcher, sim3_pair, _arr, _c_floats


class _Sim3RansacProblem(ctypes.Structure):
    """ps_sim3_ransac_problem"""
    _fields_ = [("n", ctypes.c_int32), ("x3dc1", ctypes.c_void_p), ("x3dc2", ctypes.c_void_p), ("max_err1", ctypes.c_void_p),
                ("max_err2", ctypes.c_void_p), ("k1", ctypes.c_float * 4), ("k2", ctypes.c_float * 4), ("fix_scale", ctypes.c_int32),
                ("nhyp", ctypes.c_int32), ("draws", ctypes.c_void_p), ("min_inliers", ctypes.c_int32), ("inliers", ctypes.c_void_p),
                ("model", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("first_success", ctypes.c_int32), ("best", ctypes.c_int32)]


lib.ps_sim3_ransac.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Sim3RansacProblem), ctypes.c_int]
lib.ps_sim3_ransac_iterations.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]


def ransac_iterations(probability, min_inliers, max_iterations, n):
    """SetRansacParameters (:115-139): mRansacMaxIts for n correspondences (ps_sim3_ransac_iterations)"""
    its = ctypes.c_int(0)
    check(lib.ps_sim3_ransac_iterations(float(probability), int(min_inliers), int(max_iterations), int(n), ctypes.byref(its)))
    return its.value


def gate(sigma2):
    """mvnMaxError: 9.210 * sigma2 as the reference stores it, in a size_t - truncated - and compares it, as a float"""
    return np.float32(int(9.210 * float(np.float32(sigma2))))


def sim3_ransac(matcher, problems, want_mask=True, partial_ok=False):
    """ps_sim3_ransac for a batch.  problems: list of dicts {x3dc1 [n, 3], x3dc2 [n, 3], max_err1 [n], max_err2 [n] (see gate), k1, k2
    (fx, fy, cx, cy), fix_scale, draws int32 [nhyp, 3] raw rand() values, min_inliers}.  Returns per problem a dict: inliers int32 [nhyp],
    model float32 [nhyp, 13] (s, R row-major, t), mask uint64 [nhyp, ceil(n / 64)] (want_mask), first_success, best; a problem that
    costs nothing (no hypotheses, n < min_inliers, n < 3) returns empty arrays and -1, -1; first_success = -2 marks a problem beyond
    the limits when partial_ok lets the call return after PS_ERR_CAPACITY."""
    n = len(problems)
    if n == 0:
        return []
    arr = (_Sim3RansacProblem * n)()
    keep, outs = [], []
    for i, pr in enumerate(problems):
        p = arr[i]
        a = dict(x3dc1=_arr(pr["x3dc1"], np.float32).reshape(-1, 3), x3dc2=_arr(pr["x3dc2"], np.float32).reshape(-1, 3),
                 max_err1=_arr(pr["max_err1"], np.float32).reshape(-1), max_err2=_arr(pr["max_err2"], np.float32).reshape(-1))
        m = len(a["max_err1"])
        if any(len(v) != m for v in a.values()):
            raise ValueError("the arrays of a problem differ in length")
        a["draws"] = _arr(pr["draws"], np.int32).reshape(-1, 3)
        nh = len(a["draws"])
        for k, v in a.items():
            setattr(p, k, v.ctypes.data)
        p.n = m; p.nhyp = nh
        p.k1 = _c_floats(pr["k1"], 4); p.k2 = _c_floats(pr["k2"], 4)
        p.fix_scale = 1 if pr["fix_scale"] else 0
        p.min_inliers = int(pr["min_inliers"])
        nw = (m + 63) // 64
        o = dict(inliers=np.full(max(nh, 1), -3, np.int32), model=np.full((max(nh, 1), 13), -3, np.float32))
        if want_mask:
            o["mask"] = np.full((max(nh, 1), max(nw, 1)), 0xA5A5A5A5A5A5A5A5, np.uint64)
        for k, v in o.items():
            setattr(p, k, v.ctypes.data)
        p.first_success = -3; p.best = -3
        keep.append(a); outs.append((o, m, nh, nw))
    rc = lib.ps_sim3_ransac(matcher._h, arr, n)
    if not (partial_ok and rc == -3):
        check(rc)
    res = []
    for i, (o, m, nh, nw) in enumerate(outs):
        served = o["inliers"][0] != -3 if nh > 0 else False
        k = nh if served else 0
        r = dict(inliers=o["inliers"][:k].copy(), model=o["model"][:k].copy(), first_success=int(arr[i].first_success), best=int(arr[i].best))
        if want_mask:
            r["mask"] = o["mask"][:k, :nw].copy()
        res.append(r)
    return res


def _libc_rand():
    libc = ctypes.CDLL(None)
    libc.rand.restype = ctypes.c_int
    return libc.rand


_default_matcher = None


class Sim3Solver:
    """The reference's class (include/Sim3Solver.h) over arrays.

    Sim3Solver(kf1, kf2, matched12, fix_scale): kf = dict R [3, 3], t [3] (GetRotation / GetTranslation), K4 (fx, fy, cx, cy),
    level_sigma2 (mvLevelSigma2), octave (of mvKeysUn); kf1 also points = GetMapPointMatches() per slot; matched12 = vpMatched12.  Both
    point sets are dicts of arrays over the slots: valid (non-null), pos [.., 3], bad, index (GetIndexInKeyFrame in the point's own
    keyframe).  matcher: the ORBmatcher whose handle runs the call (one is created when none is given); rand: the source of raw rand()
    values, libc's rand() by default.  from_arrays takes mvX3Dc1 / mvX3Dc2, the gates and mvnIndices1 outright."""

    def __init__(self, kf1, kf2, matched12, fix_scale, matcher=None, rand=None):
        p1, p2 = kf1["points"], matched12
        n1 = len(p2["valid"])
        v = lambda d, k, dt: np.asarray(d[k], dt)[:n1]
        idx1, idx2 = v(p1, "index", np.int64), v(p2, "index", np.int64)
        ok = (v(p2, "valid", bool) & v(p1, "valid", bool) & ~v(p1, "bad", bool) & ~v(p2, "bad", bool) & (idx1 >= 0) & (idx2 >= 0))   # :65-80
        sel = np.nonzero(ok)[0]
        s1 = np.asarray(kf1["level_sigma2"], np.float32)[np.asarray(kf1["octave"], np.int64)[idx1[sel]]]
        s2 = np.asarray(kf2["level_sigma2"], np.float32)[np.asarray(kf2["octave"], np.int64)[idx2[sel]]]
        g1 = np.array([gate(s) for s in s1], np.float32)
        g2 = np.array([gate(s) for s in s2], np.float32)
        x1 = self._to_camera(kf1, np.asarray(p1["pos"], np.float32).reshape(-1, 3)[sel])
        x2 = self._to_camera(kf2, np.asarray(p2["pos"], np.float32).reshape(-1, 3)[sel])
        self._setup(x1, x2, g1, g2, kf1["K4"], kf2["K4"], sel, n1, fix_scale, matcher, rand)

    @classmethod
    def from_arrays(cls, x3dc1, x3dc2, max_err1, max_err2, k1, k2, fix_scale, indices1=None, n1=None, matcher=None, rand=None):
        self = cls.__new__(cls)
        n = len(np.asarray(max_err1).reshape(-1))
        self._setup(x3dc1, x3dc2, max_err1, max_err2, k1, k2, np.arange(n) if indices1 is None else indices1, n if n1 is None else n1,
                    fix_scale, matcher, rand)
        return self

    @staticmethod
    def _to_camera(kf, X):
        """Rcw * X3Dw + tcw (:96, :99): the product's terms and their sum in double, rounded, then the float addition"""
        R = np.asarray(kf["R"], np.float32).reshape(3, 3)
        t = np.asarray(kf["t"], np.float32).reshape(3)
        Xd = X.astype(np.float64)
        out = np.zeros((len(X), 3), np.float32)
        for r in range(3):
            out[:, r] = ((float(R[r, 0]) * Xd[:, 0] + float(R[r, 1]) * Xd[:, 1]) + float(R[r, 2]) * Xd[:, 2]).astype(np.float32) + t[r]
        return out

    def _setup(self, x1, x2, g1, g2, k1, k2, indices1, n1, fix_scale, matcher, rand):
        self.mvX3Dc1 = _arr(x1, np.float32).reshape(-1, 3); self.mvX3Dc2 = _arr(x2, np.float32).reshape(-1, 3)
        self.mvnMaxError1 = _arr(g1, np.float32).reshape(-1); self.mvnMaxError2 = _arr(g2, np.float32).reshape(-1)
        self.mK1 = np.asarray(k1, np.float32).reshape(4); self.mK2 = np.asarray(k2, np.float32).reshape(4)
        self.mvnIndices1 = np.asarray(indices1, np.int64).reshape(-1)
        self.mN1 = int(n1)
        self.mbFixScale = bool(fix_scale)
        self.matcher = matcher
        self.rand = rand
        self.mnBestInliers = 0
        self._best = -1
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.mRansacProb = float(probability); self.mRansacMinInliers = int(minInliers)
        self.N = len(self.mvnMaxError1)
        self.mRansacMaxIts = ransac_iterations(probability, minInliers, maxIterations, self.N)
        self.mnIterations = 0
        self._res = None          # the cached hypotheses: not prepared

    def _live(self):
        return self.N >= self.mRansacMinInliers and self.N >= 3

    @staticmethod
    def PrepareBatch(solvers, matcher=None):
        """all mRansacMaxIts hypotheses of every live, un-prepared solver in one ps_sim3_ransac"""
        global _default_matcher
        todo = [s for s in solvers if s is not None and s._res is None and s._live()]
        if not todo:
            return
        m = matcher or next((s.matcher for s in todo if s.matcher is not None), None)
        if m is None:
            if _default_matcher is None:
                _default_matcher = ORBmatcher()
            m = _default_matcher
        probs = []
        for s in todo:
            rand = s.rand or _libc_rand()
            draws = np.array([rand() for _ in range(3 * s.mRansacMaxIts)], np.int32).reshape(-1, 3)
            probs.append(dict(x3dc1=s.mvX3Dc1, x3dc2=s.mvX3Dc2, max_err1=s.mvnMaxError1, max_err2=s.mvnMaxError2, k1=s.mK1, k2=s.mK2,
                              fix_scale=s.mbFixScale, draws=draws, min_inliers=s.mRansacMinInliers))
        for s, r in zip(todo, sim3_ransac(m, probs)):
            s._res = r

    def _take(self, h):
        m = self._res["model"][h]
        self._best = h
        self.mnBestInliers = int(self._res["inliers"][h])
        self.mBestScale = np.float32(m[0]); self.mBestRotation = m[1:10].reshape(3, 3).copy(); self.mBestTranslation = m[10:13].copy()
        sR12, t12, _, _ = sim3_pair(m[0], self.mBestRotation, self.mBestTranslation)
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = sR12; T[:3, 3] = t12
        self.mBestT12 = T

    def iterate(self, nIterations):
        """-> (T12 float32 [4, 4] or None, bNoMore, vbInliers bool [mN1], nInliers) exactly as :141-208"""
        vbInliers = np.zeros(self.mN1, bool)
        if not self._live():      # (fewer than three correspondences: the reference's draw is undefined)
            return None, True, vbInliers, 0
        if self._res is None:
            Sim3Solver.PrepareBatch([self])
        inl = self._res["inliers"]
        done = 0
        while self.mnIterations < self.mRansacMaxIts and done < nIterations:
            h = self.mnIterations
            done += 1
            self.mnIterations += 1
            c = int(inl[h])
            if c >= self.mnBestInliers:
                self._take(h)
                if c > self.mRansacMinInliers:
                    words = self._res["mask"][h]
                    i = np.arange(self.N)
                    bits = ((words[i >> 6] >> (i & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
                    vbInliers[self.mvnIndices1[bits]] = True
                    return self.mBestT12.copy(), False, vbInliers, c
        return None, self.mnIterations >= self.mRansacMaxIts, vbInliers, 0

    def find(self):
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n

    def GetEstimatedRotation(self):
        return self.mBestRotation.copy() if self._best >= 0 else None

    def GetEstimatedTranslation(self):
        return self.mBestTranslation.copy() if self._best >= 0 else None

    def GetEstimatedScale(self):
        return self.mBestScale if self._best >= 0 else None
