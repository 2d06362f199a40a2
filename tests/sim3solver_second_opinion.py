"""A literal, sequential restatement of ORB_SLAM2::Sim3Solver (/root/reference/src/Sim3Solver.cc) in numpy - the second opinion the
device solver (ps_sim3_ransac, pointslot_amd.Sim3Solver) is compared against.  Nothing here shares code with the package.

The evaluation type of every expression is written out: F(..) is a float32 rounding, D(..) a double.
  constructor (:38-113)        the skip rules, mvnIndices1, Rcw * X + tcw (the product's three terms and their sum in double, rounded,
                               then a float addition - the convention of the projection matchers), 9.210 * sigma2 stored in a size_t
  SetRansacParameters (:115-139)  with its float epsilon; a quotient that does not fit an int converts as x86 does (INT_MIN)
  iterate (:141-208)           with its std::vector draw loop and DUtils::Random::RandomInt on raw rand() values
  ComputeSim3 (:227-338)       centroids and relative coordinates float32 (cv::reduce sums in float, C / 3 = F(D(C) * (1.0 / 3.0)));
                               M = Pr2 * Pr1^T with products and sum in double, rounded once; the ten sums of N in double, each
                               rounded to float32; the eigenvector of that float32 N in FP64 (numpy.linalg.eigh, or the plain cyclic
                               Jacobi below), sign q0 >= 0, rounded to float32; ang = atan2(norm(vec), q0) in double;
                               vec = 2 * ang * vec / norm(vec) as one scale (2 ang) * (1 / norm) on D(vec), rounded once;
                               cv::Rodrigues in double, R = c I + (1 - c) r r^T + s [r]x, rounded to float32; P3 = R * Pr2;
                               nom = Pr1.dot(P3) in double, den the double sum of the float squares; ms12i = F(nom / den);
                               t12 = F(D(O1) - D(s) * (R O2 in double)); T12 / T21 as pointslot_amd.matcher.sim3_pair states them
  CheckInliers / Project / FromCameraToImage (:341-424)   float32 as written, err = F(dot in double), no positivity test on z
"""
import numpy as np

F = np.float32
D = np.float64
RAND_MAX = 2147483647


def random_int(r, size):
    """DUtils::Random::RandomInt(0, size - 1) on the raw rand() value r"""
    return int((float(r) / (float(RAND_MAX) + 1.0)) * size)


def draw_triple_list(r3, n):
    """:164-178 as written: the list of available indices, pick, move the back element into the slot, pop"""
    avail = list(range(n))
    out = []
    for i in range(3):
        randi = random_int(r3[i], len(avail))
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


def draw_triple_closed(r3, n):
    """the same three indices without a list"""
    r0, r1, r2 = random_int(r3[0], n), random_int(r3[1], n - 1), random_int(r3[2], n - 2)
    i1 = n - 1 if r1 == r0 else r1
    back = n - 1 if n - 2 == r0 else n - 2
    i2 = back if r2 == r1 else (n - 1 if r2 == r0 else r2)
    return [r0, i1, i2]


def ransac_iterations(probability, min_inliers, max_iterations, n):
    """SetRansacParameters: mRansacMaxIts"""
    with np.errstate(all="ignore"):
        epsilon = F(min_inliers) / F(n)
        if min_inliers == n:
            its = 1
        else:
            v = np.ceil(np.log(D(1) - D(probability)) / np.log(D(1) - np.power(D(epsilon), D(3.0))))
            its = int(v) if np.isfinite(v) and -2147483648.0 <= v < 2147483648.0 else -2147483648
    return max(1, min(its, max_iterations))


def _dotd(a, b):
    """float32 vectors: products and their sum in double, left to right"""
    s = D(a[0]) * D(b[0])
    for k in range(1, len(a)):
        s = s + D(a[k]) * D(b[k])
    return s


def jacobi_eig4(N):
    """plain cyclic Jacobi on a symmetric 4x4 in FP64 -> (eigenvalues [4], eigenvectors as columns [4, 4]), unsorted"""
    with np.errstate(all="ignore"):
        A = [[D(N[i][j]) for j in range(4)] for i in range(4)]
        V = [[D(1.0 if i == j else 0.0) for j in range(4)] for i in range(4)]
        for _ in range(16):
            off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3]
            dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3]
            if off <= D(1e-40) * dia:
                break
            for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = D(0.5) * (A[q][q] - A[p][p]) / apq
                t = D(1.0) / (np.abs(theta) + np.sqrt(theta * theta + D(1.0)))
                if theta < 0.0:
                    t = -t
                c = D(1.0) / np.sqrt(t * t + D(1.0))
                s = t * c
                tau = s / (D(1.0) + c)
                h = t * apq
                A[p][p] = A[p][p] - h
                A[q][q] = A[q][q] + h
                A[p][q] = A[q][p] = D(0.0)
                for k in range(4):
                    if k != p and k != q:
                        g, e = A[k][p], A[k][q]
                        A[k][p] = A[p][k] = g - s * (e + g * tau)
                        A[k][q] = A[q][k] = e + s * (g - e * tau)
                for k in range(4):
                    g, e = V[k][p], V[k][q]
                    V[k][p] = g - s * (e + g * tau)
                    V[k][q] = e + s * (g - e * tau)
    return np.array([A[i][i] for i in range(4)], D), np.array(V, D)


def top_eigenvector(N32, solver):
    """the eigenvector of the largest eigenvalue of the float32 N in FP64, q0 >= 0 -> (q float64 [4], gap ratio)"""
    Nd = np.asarray(N32, F).astype(D)
    if solver == "eigh":
        w, v = np.linalg.eigh(Nd)
        q = v[:, 3].copy()
        ws = w
    else:
        w, v = jacobi_eig4(Nd)
        k = 0
        for i in range(1, 4):
            if w[i] > w[k]:
                k = i
        q = v[:, k].copy()
        ws = np.sort(w)
    if q[0] < 0.0:
        q = -q
    with np.errstate(all="ignore"):
        gap = (ws[3] - ws[2]) / np.abs(ws[3])
    return q, float(gap)


def compute_sim3(P1, P2, fix_scale, solver="eigh"):
    """ComputeSim3 on float32 P1, P2 [3, 3] (column i = point i) -> dict: s, R, t, sR12, t12, sR21, t21 (float32), N, gap"""
    P1 = np.asarray(P1, F)
    P2 = np.asarray(P2, F)
    with np.errstate(all="ignore"):
        O1 = np.zeros(3, F); O2 = np.zeros(3, F)
        Pr1 = np.zeros((3, 3), F); Pr2 = np.zeros((3, 3), F)
        for r in range(3):
            O1[r] = F(D(F(F(P1[r, 0] + P1[r, 1]) + P1[r, 2])) * (D(1.0) / D(3.0)))
            O2[r] = F(D(F(F(P2[r, 0] + P2[r, 1]) + P2[r, 2])) * (D(1.0) / D(3.0)))
            for i in range(3):
                Pr1[r, i] = F(P1[r, i] - O1[r])
                Pr2[r, i] = F(P2[r, i] - O2[r])
        M = np.zeros((3, 3), F)
        for r in range(3):
            for c in range(3):
                M[r, c] = F(_dotd(Pr2[r], Pr1[c]))
        m = M.astype(D)
        N11 = F(m[0, 0] + m[1, 1] + m[2, 2]); N12 = F(m[1, 2] - m[2, 1]); N13 = F(m[2, 0] - m[0, 2]); N14 = F(m[0, 1] - m[1, 0])
        N22 = F(m[0, 0] - m[1, 1] - m[2, 2]); N23 = F(m[0, 1] + m[1, 0]); N24 = F(m[2, 0] + m[0, 2])
        N33 = F(-m[0, 0] + m[1, 1] - m[2, 2]); N34 = F(m[1, 2] + m[2, 1]); N44 = F(-m[0, 0] - m[1, 1] + m[2, 2])
        N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], F)
        q, gap = top_eigenvector(N, solver)
        e = q.astype(F)
        nrm = np.sqrt(D(e[1]) * D(e[1]) + D(e[2]) * D(e[2]) + D(e[3]) * D(e[3]))
        ang = np.arctan2(nrm, D(e[0]))
        a = (D(2.0) * ang) * (D(1.0) / nrm)
        vec = np.array([F(D(e[1]) * a), F(D(e[2]) * a), F(D(e[3]) * a)], F)
        # cv::Rodrigues
        rv = vec.astype(D)
        theta = np.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2])
        R = np.zeros((3, 3), F)
        if theta < np.finfo(D).eps:
            R[:] = np.eye(3, dtype=F)
        else:
            c, s = np.cos(theta), np.sin(theta)
            c1 = D(1.0) - c
            it = D(1.0) / theta
            rx, ry, rz = rv[0] * it, rv[1] * it, rv[2] * it
            ru = (rx, ry, rz)
            cr = ((D(0.0), -rz, ry), (rz, D(0.0), -rx), (-ry, rx, D(0.0)))
            for r in range(3):
                for k in range(3):
                    R[r, k] = F((c * D(1.0 if r == k else 0.0) + c1 * (ru[r] * ru[k])) + s * cr[r][k])
        if not fix_scale:
            nom = D(0.0); den = D(0.0)
            for r in range(3):
                for i in range(3):
                    p3 = F(_dotd(R[r], Pr2[:, i]))
                    nom = nom + D(Pr1[r, i]) * D(p3)
                    den = den + D(F(p3 * p3))
            s12 = F(nom / den)
        else:
            s12 = F(1.0)
        sd = D(s12)
        inv = D(1.0) / D(s12)
        t12 = np.zeros(3, F); sR12 = np.zeros((3, 3), F); sR21 = np.zeros((3, 3), F); t21 = np.zeros(3, F)
        for r in range(3):
            t12[r] = F(D(O1[r]) - sd * _dotd(R[r], O2))
            for c in range(3):
                sR12[r, c] = F(D(R[r, c]) * sd)
                sR21[r, c] = F(D(R[c, r]) * inv)
        for r in range(3):
            t21[r] = F(-_dotd(sR21[r], t12))
    return dict(s=s12, R=R, t=t12, sR12=sR12, t12=t12, sR21=sR21, t21=t21, N=N, gap=gap)


def model13(mod):
    return np.concatenate([[mod["s"]], mod["R"].reshape(9), mod["t"]]).astype(F)


def pair_from_model13(m13):
    """T12 / T21 of a float32 model (s, R, t) as ComputeSim3's step 8 states them"""
    m13 = np.asarray(m13, F)
    s12, R, t12 = m13[0], m13[1:10].reshape(3, 3), m13[10:13]
    with np.errstate(all="ignore"):
        sd = D(s12); inv = D(1.0) / D(s12)
        sR12 = (R.astype(D) * sd).astype(F)
        sR21 = (R.T.astype(D) * inv).astype(F)
        t21 = np.array([F(-_dotd(sR21[r], t12)) for r in range(3)], F)
    return sR12, t12.copy(), sR21, t21


def from_camera_to_image(X, k4):
    """FromCameraToImage on float32 X [n, 3] -> (u, v) float32"""
    X = np.asarray(X, F).reshape(-1, 3)
    fx, fy, cx, cy = [F(v) for v in k4]
    with np.errstate(all="ignore"):
        invz = F(1.0) / X[:, 2]
        x = X[:, 0] * invz
        y = X[:, 1] * invz
        return fx * x + cx, fy * y + cy


def project(X, sR, t, k4):
    """Project: Rcw * X + tcw (products and sum in double, rounded, then the float addition), then as FromCameraToImage"""
    X = np.asarray(X, F).reshape(-1, 3)
    Xd = X.astype(D)
    P = np.zeros_like(X)
    with np.errstate(all="ignore"):
        for r in range(3):
            P[:, r] = ((D(sR[r, 0]) * Xd[:, 0] + D(sR[r, 1]) * Xd[:, 1]) + D(sR[r, 2]) * Xd[:, 2]).astype(F) + F(t[r])
    return from_camera_to_image(P, k4)


def check_inliers(x1, x2, g1, g2, k1, k2, sR12, t12, sR21, t21, return_err=False):
    """CheckInliers -> mvbInliersi (bool [n])"""
    u1, v1 = from_camera_to_image(x1, k1)       # mvP1im1
    u2, v2 = from_camera_to_image(x2, k2)       # mvP2im2
    a, b = project(x2, sR12, t12, k1)           # vP2im1
    c, d = project(x1, sR21, t21, k2)           # vP1im2
    with np.errstate(all="ignore"):
        d0, d1 = u1 - a, v1 - b
        e0, e1 = c - u2, d - v2
        err1 = (d0.astype(D) * d0.astype(D) + d1.astype(D) * d1.astype(D)).astype(F)
        err2 = (e0.astype(D) * e0.astype(D) + e1.astype(D) * e1.astype(D)).astype(F)
        inl = (err1 < np.asarray(g1, F)) & (err2 < np.asarray(g2, F))
    return (inl, err1, err2) if return_err else inl


def mask_words(inl):
    n = len(inl)
    w = np.zeros((n + 63) // 64, np.uint64)
    for i in np.nonzero(inl)[0]:
        w[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return w


def gate(sigma2):
    """mvnMaxError.push_back(9.210 * sigmaSquare): a double stored in a size_t, compared as a float"""
    return F(int(9.210 * float(F(sigma2))))


class Sim3SolverRef:
    """The class as the reference runs it.  rand: a callable returning raw rand() values; solver: "eigh" or "jacobi"."""

    def __init__(self, kf1, kf2, matched12, fix_scale, rand, solver="eigh"):
        """kf: dict R [3, 3], t [3], K4, level_sigma2, octave (of mvKeysUn); kf1 also points = the keyframe's map points per slot;
        matched12 = vpMatched12.  A point is None or a dict pos [3], bad, index (GetIndexInKeyFrame in its own keyframe)."""
        self.mnIterations = 0; self.mnBestInliers = 0; self.mbFixScale = bool(fix_scale)
        self.rand = rand; self.solver = solver
        self.mN1 = len(matched12)
        self.mvnIndices1 = []; x1 = []; x2 = []; g1 = []; g2 = []
        for i1 in range(self.mN1):
            if matched12[i1] is not None:
                p1, p2 = kf1["points"][i1], matched12[i1]
                if p1 is None:
                    continue
                if p1["bad"] or p2["bad"]:
                    continue
                if p1["index"] < 0 or p2["index"] < 0:
                    continue
                g1.append(gate(kf1["level_sigma2"][kf1["octave"][p1["index"]]]))
                g2.append(gate(kf2["level_sigma2"][kf2["octave"][p2["index"]]]))
                self.mvnIndices1.append(i1)
                x1.append(self._to_camera(kf1, p1["pos"]))
                x2.append(self._to_camera(kf2, p2["pos"]))
        self._arrays(x1, x2, g1, g2, kf1["K4"], kf2["K4"])
        self.SetRansacParameters()

    @classmethod
    def from_arrays(cls, x3dc1, x3dc2, max_err1, max_err2, k1, k2, fix_scale, rand, indices1=None, n1=None, solver="eigh"):
        self = cls.__new__(cls)
        self.mnIterations = 0; self.mnBestInliers = 0; self.mbFixScale = bool(fix_scale)
        self.rand = rand; self.solver = solver
        n = len(max_err1)
        self.mvnIndices1 = list(range(n)) if indices1 is None else [int(i) for i in indices1]
        self.mN1 = n if n1 is None else int(n1)
        self._arrays(x3dc1, x3dc2, max_err1, max_err2, k1, k2)
        self.SetRansacParameters()
        return self

    @staticmethod
    def _to_camera(kf, pos):
        R = np.asarray(kf["R"], F).reshape(3, 3); t = np.asarray(kf["t"], F).reshape(3); X = np.asarray(pos, F).reshape(3)
        return np.array([F(F(_dotd(R[r], X)) + t[r]) for r in range(3)], F)

    def _arrays(self, x1, x2, g1, g2, k1, k2):
        self.mvX3Dc1 = np.asarray(x1, F).reshape(-1, 3); self.mvX3Dc2 = np.asarray(x2, F).reshape(-1, 3)
        self.mvnMaxError1 = np.asarray(g1, F).reshape(-1); self.mvnMaxError2 = np.asarray(g2, F).reshape(-1)
        self.mK1 = np.asarray(k1, F); self.mK2 = np.asarray(k2, F)

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.mRansacProb = probability; self.mRansacMinInliers = minInliers
        self.N = len(self.mvnMaxError1)
        self.mvbInliersi = np.zeros(self.N, bool)
        self.mRansacMaxIts = ransac_iterations(probability, minInliers, maxIterations, self.N)
        self.mnIterations = 0

    def hypothesis(self, idx):
        """ComputeSim3 + CheckInliers on the three correspondences idx -> (model dict, mvbInliersi)"""
        mod = compute_sim3(self.mvX3Dc1[idx].T, self.mvX3Dc2[idx].T, self.mbFixScale, self.solver)
        inl = check_inliers(self.mvX3Dc1, self.mvX3Dc2, self.mvnMaxError1, self.mvnMaxError2, self.mK1, self.mK2,
                            mod["sR12"], mod["t12"], mod["sR21"], mod["t21"])
        return mod, inl

    def evaluate(self, idx):
        """what iterate does with one hypothesis; tests replace this to feed recorded counts"""
        mod, inl = self.hypothesis(idx)
        return model13(mod), inl, int(inl.sum())

    def iterate(self, nIterations):
        """-> (model13 or None, bNoMore, vbInliers bool [mN1], nInliers)"""
        bNoMore = False
        vbInliers = np.zeros(self.mN1, bool)
        nInliers = 0
        if self.N < self.mRansacMinInliers:
            return None, True, vbInliers, nInliers
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts and nCurrentIterations < nIterations:
            nCurrentIterations += 1
            self.mnIterations += 1
            idx = draw_triple_list([self.rand(), self.rand(), self.rand()], self.N)
            m13, inl, cnt = self.evaluate(idx)
            if cnt >= self.mnBestInliers:
                self.mvbBestInliers = inl.copy(); self.mnBestInliers = cnt; self.mBest = m13
                if cnt > self.mRansacMinInliers:
                    nInliers = cnt
                    for i in range(self.N):
                        if inl[i]:
                            vbInliers[self.mvnIndices1[i]] = True
                    return m13, bNoMore, vbInliers, nInliers
        if self.mnIterations >= self.mRansacMaxIts:
            bNoMore = True
        return None, bNoMore, vbInliers, nInliers

    def find(self):
        m, _, vb, n = self.iterate(self.mRansacMaxIts)
        return m, vb, n


def run_all(case, solver="eigh", with_err=False):
    """every hypothesis of a case (tests/sim3solver_cases.py) -> dict inliers [nhyp], model [nhyp, 13], mask [nhyp, nwords], gap [nhyp],
    idx [nhyp, 3] (and err1 / err2 [nhyp, n] with with_err)"""
    n, nhyp = case["n"], len(case["draws"])
    out = dict(inliers=np.zeros(nhyp, np.int32), model=np.zeros((nhyp, 13), F), mask=np.zeros((nhyp, (n + 63) // 64), np.uint64),
               gap=np.zeros(nhyp), idx=np.zeros((nhyp, 3), np.int32))
    if with_err:
        out["err1"] = np.zeros((nhyp, n), F); out["err2"] = np.zeros((nhyp, n), F)
    for h in range(nhyp):
        idx = draw_triple_list(case["draws"][h], n)
        mod = compute_sim3(case["x3dc1"][idx].T, case["x3dc2"][idx].T, case["fix_scale"], solver)
        r = check_inliers(case["x3dc1"], case["x3dc2"], case["max_err1"], case["max_err2"], case["k1"], case["k2"],
                          mod["sR12"], mod["t12"], mod["sR21"], mod["t21"], return_err=with_err)
        inl = r[0] if with_err else r
        if with_err:
            out["err1"][h], out["err2"][h] = r[1], r[2]
        out["inliers"][h] = int(inl.sum()); out["model"][h] = model13(mod); out["mask"][h] = mask_words(inl); out["gap"][h] = mod["gap"]
        out["idx"][h] = idx
    return out


def sequence_outcome(inliers, min_inliers):
    """(first_success, best) of a list of counts by iterate's own bookkeeping over all hypotheses"""
    best_n, best, first = 0, -1, -1
    for h, c in enumerate(inliers):
        if c >= best_n:
            best_n, best = c, h
        if first < 0 and c > min_inliers:
            first = h
    return first, best
