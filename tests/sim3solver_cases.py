"""Seeded cases for the Sim3 solver (ps_sim3_ransac, pointslot_amd.Sim3Solver), as small as the failure modes allow.  A case is the
input of one problem of the call: n, x3dc1 / x3dc2 float32 [n, 3], max_err1 / max_err2 (truncated gates), k1 / k2, fix_scale,
draws int32 [nhyp, 3] (raw rand() values), min_inliers; `full1` / `full2` are the untruncated 9.210 * sigma2 and `degenerate` marks the
cases that are compared on counts only.  CASES is built once at import."""
import numpy as np

F = np.float32
RAND_MAX = 2147483647
K1 = (721.5377, 721.5377, 609.5593, 172.854)
K2 = (718.856, 718.856, 607.1928, 185.2157)
TILE = 512          # PS_S3_TILE: correspondences per LDS tile
NHYP = 300


def raw_for(k, size):
    """a raw rand() value that DUtils::Random::RandomInt(0, size - 1) maps to k"""
    return int((k + 0.5) * 2147483648.0 / size)


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def scene(seed, n, outliers, noise, fix_scale, min_inliers=6, nhyp=NHYP, scale=None, behind=0):
    """n correspondences seen by two cameras related by a similarity; a share of them wrong; gates from random octaves"""
    rng = np.random.RandomState(seed)
    z = rng.uniform(4, 30, n)
    X1 = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.2, 0.2, n) * z, z], 1)
    s = 1.0 if fix_scale else (scale or rng.uniform(0.8, 1.25))
    R12 = _rot(rng.normal(size=3), rng.uniform(0.02, 0.25))
    t12 = rng.uniform(-1.0, 1.0, 3)
    X2 = ((X1 - t12) @ R12) / s                      # X1 = s R12 X2 + t12
    X1 = X1 + rng.normal(size=X1.shape) * noise * z[:, None] / 720.0
    X2 = X2 + rng.normal(size=X2.shape) * noise * z[:, None] / 720.0
    bad = rng.permutation(n)[:int(round(outliers * n))]
    zb = rng.uniform(4, 30, len(bad))
    X2[bad] = np.stack([rng.uniform(-0.6, 0.6, len(bad)) * zb, rng.uniform(-0.2, 0.2, len(bad)) * zb, zb], 1)
    if behind:
        X2[bad[:behind], 2] = -rng.uniform(0.5, 5, behind)       # points behind camera 2: invz has no positivity test
        X1[bad[behind:2 * behind], 2] = -rng.uniform(0.5, 5, behind)
    sig1 = (F(1.2) ** rng.randint(0, 8, n).astype(F)) ** 2
    sig2 = (F(1.2) ** rng.randint(0, 8, n).astype(F)) ** 2
    full1 = 9.210 * sig1.astype(F).astype(float)
    full2 = 9.210 * sig2.astype(F).astype(float)
    return dict(n=n, x3dc1=X1.astype(F), x3dc2=X2.astype(F), max_err1=np.floor(full1).astype(F), max_err2=np.floor(full2).astype(F),
                full1=full1, full2=full2, k1=K1, k2=K2, fix_scale=int(fix_scale), min_inliers=min_inliers,
                draws=rng.randint(0, RAND_MAX, (nhyp, 3)).astype(np.int32), degenerate=False)


def _build():
    C = {}
    # sizes: below / at / past a wave, several ballots, one LDS tile crossed by one
    C["n21"] = scene(1, 21, 0.3, 0.4, False)
    C["n40_fix"] = scene(2, 40, 0.5, 0.4, True, min_inliers=10)
    C["n64"] = scene(3, 64, 0.4, 0.4, False, min_inliers=20)
    C["n65_fix"] = scene(4, 65, 0.4, 0.4, True, min_inliers=20)
    C["n150"] = scene(5, 150, 0.5, 0.5, False, min_inliers=20)
    C["n300_fix"] = scene(6, 300, 0.45, 0.5, True, min_inliers=20)
    C["tile_plus_1"] = scene(7, TILE + 1, 0.5, 0.5, False, min_inliers=20)
    # the draw rule by hand: hypothesis 0 draws slot 5 and then slot 5 again (which now holds the moved back element, n - 1);
    # hypothesis 1: r = RAND_MAX three times (always the last slot); hypothesis 2: first n - 2 (so the back element at the second
    # removal is n - 1), then the slot drawn second again; hypothesis 3: the third draw lands on the first draw's slot
    d = scene(8, 21, 0.2, 0.3, False, nhyp=8)
    n = 21
    d["draws"][0] = [raw_for(5, n), raw_for(5, n - 1), raw_for(0, n - 2)]
    d["draws"][1] = [RAND_MAX, RAND_MAX, RAND_MAX]
    d["draws"][2] = [raw_for(n - 2, n), raw_for(3, n - 1), raw_for(3, n - 2)]
    d["draws"][3] = [raw_for(7, n), raw_for(2, n - 1), raw_for(7, n - 2)]
    d["draws"][4] = [0, 0, 0]
    C["draw_rule"] = d
    # pure translation on exactly representable coordinates (multiples of 0.75, so the centroids are exact): Pr1 == Pr2 bit for
    # bit, M is symmetric, the quaternion is (1, 0, 0, 0) and the reference computes 0 * (1 / 0) = NaN
    rng = np.random.RandomState(9)
    n = 40
    X2 = np.stack([rng.randint(-12, 13, n) * 0.75, rng.randint(-4, 5, n) * 0.75, rng.randint(6, 40, n) * 0.75], 1)
    X1 = X2 + np.array([1.5, -0.75, 2.25])
    g = np.full(n, 9.0, F)
    C["pure_translation"] = dict(n=n, x3dc1=X1.astype(F), x3dc2=X2.astype(F), max_err1=g, max_err2=g.copy(), full1=g * 0 + 9.21, full2=g * 0 + 9.21,
                                 k1=K1, k2=K2, fix_scale=0, min_inliers=6, draws=rng.randint(0, RAND_MAX, (60, 3)).astype(np.int32), degenerate=True)
    C["behind_camera"] = scene(10, 64, 0.4, 0.4, False, min_inliers=20, behind=6)
    # a near-collinear triple (points 0, 1, 2), drawn by hand in hypothesis 0 and, reordered, in hypothesis 1
    d = scene(11, 40, 0.3, 0.4, False, nhyp=40)
    base, step = d["x3dc1"][0].astype(float), np.array([0.9, 0.2, 1.3])
    for k in (1, 2):
        d["x3dc1"][k] = (base + k * step + 1e-5 * np.array([k, -k, 0.5])).astype(F)
    n = 40
    d["draws"][0] = [raw_for(0, n), raw_for(1, n - 1), raw_for(2, n - 2)]
    d["draws"][1] = [raw_for(2, n), raw_for(1, n - 1), raw_for(0, n - 2)]
    d["degenerate"] = True
    C["near_collinear"] = d
    # reprojection errors around the gates: many decisions fall between the truncated gate and 9.210 * sigma2
    C["gates"] = scene(12, 150, 0.3, 2.2, False, min_inliers=20)
    # boundaries
    C["n_eq_min"] = scene(13, 21, 0.2, 0.3, False, min_inliers=21)
    C["n_lt_min"] = scene(14, 18, 0.2, 0.3, False, min_inliers=20)
    # no success in 300: `best` with ties decides
    # (the second half of the draws repeats the first, so the maximum is attained at least twice)
    C["no_success"] = scene(15, 40, 0.7, 3.0, True, min_inliers=30)
    C["no_success"]["draws"][150:] = C["no_success"]["draws"][:150]
    return C


CASES = _build()
SOLVABLE = ["n21", "n40_fix", "n64", "n65_fix", "n150", "n300_fix", "tile_plus_1", "behind_camera", "gates"]
RAGGED = ["n21", "n65_fix", "n_lt_min", "tile_plus_1", "pure_translation", "draw_rule", "no_success", "n150"]


def problem(case):
    return {k: case[k] for k in ("x3dc1", "x3dc2", "max_err1", "max_err2", "k1", "k2", "fix_scale", "draws", "min_inliers")}


_EXPECTED = {}


def expected(name, solver="eigh"):
    """the restatement's run over every hypothesis of a case (sim3solver_second_opinion.run_all), computed once and shared: treat as
    read-only"""
    key = (name, solver)
    if key not in _EXPECTED:
        import sim3solver_second_opinion as so
        _EXPECTED[key] = so.run_all(CASES[name], solver, with_err=(name == "gates"))
    return _EXPECTED[key]
