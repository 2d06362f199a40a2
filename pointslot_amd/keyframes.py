"""Seeded keyframe sets for LocalMapping::CreateNewMapPoints (ps_create_new_map_points): a current keyframe and its neighbours on
a forward drive, 3-D points seen from several of them with pixel noise, stereo measurements for the near points, descriptors
with a few flipped bits per view, vocabulary-node ids shared between the views (a configurable share mislabelled or missing)
and pre-occupied slots.  Pure numpy on pointslot_amd.synth's generator, so every consumer sees identical bytes."""
import numpy as np

from . import synth

F32 = np.float32
KITTI_K = (718.856, 718.856, 607.1928, 185.2157)
KITTI_BF = 386.1448


def compute_f12(kf1, kf2):
    """LocalMapping::ComputeF12 (/root/reference/src/LocalMapping.cc:804-823): K1^-T [t12]x R12 K2^-1, float32 [3, 3] with
    x1^T F12 x2 = 0.  Host glue - the caller's in the C-ABI; evaluated in float64 here and rounded once."""
    R1, t1 = np.asarray(kf1["R"], np.float64).reshape(3, 3), np.asarray(kf1["t"], np.float64).reshape(3)
    R2, t2 = np.asarray(kf2["R"], np.float64).reshape(3, 3), np.asarray(kf2["t"], np.float64).reshape(3)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])

    def kmat(kf):
        fx, fy, cx, cy = [float(v) for v in kf["K8"][:4]]
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    return (np.linalg.inv(kmat(kf1)).T @ tx @ R12 @ np.linalg.inv(kmat(kf2))).astype(F32)


def keyframe_set(seed, n_kf=4, n=300, n_nodes=12, step=1.0, noise=0.5, flip_bits=10, p_wrong=0.1, p_none=0.05, p_occupied=0.25,
                 p_seen=0.85, stereo_depth=25.0, p_stereo=0.85, raw_shift=0.0, w=1241, h=376, sizes=None, descriptor_families=None):
    """n_kf keyframes; [0] is the current one, [i] lies about i * step metres behind it (step: a sequence gives one distance per
    keyframe instead).  Every keyframe has n features (sizes: one count per keyframe instead): projections of shared world
    points where enough are visible, random clutter otherwise, in an order of the keyframe's own.  raw_shift: mvKeys differ from
    mvKeysUn by that many pixels (x_raw, y_raw); 0 leaves them out.  descriptor_families = (families, members, spread): the first
    families * members world points come in groups that share a vocabulary node and a base descriptor, each member up to `spread`
    bits away from it - repetitive texture, where the nearest and the second nearest candidate are close (independent random
    descriptors are about 128 bits apart, and no ratio test or already-matched rule ever decides anything).  Off by default; it
    draws from a generator of its own, so the bytes of every other configuration stay as they are."""
    rng = synth.Rng(seed)
    fx, fy, cx, cy = KITTI_K
    sig, _ = synth._level_sigma()
    sizes = [n] * n_kf if sizes is None else list(sizes)
    npts = int(max(sizes + [1]) * 2)
    # world points ahead of the current keyframe; the camera looks along +z
    zw = rng.uniform(npts, 5.0, 45.0)
    xw = rng.uniform(npts, -0.55, 0.55) * zw
    yw = rng.uniform(npts, -0.2, 0.2) * zw
    P = np.stack([xw, yw, zw], 1)
    base_desc = rng.integers(npts * 32, 0, 256).astype(np.uint8).reshape(npts, 32)
    base_oct = np.searchsorted(np.cumsum(synth._QUOTAS) / synth._QUOTAS.sum(), rng.uniform(npts)).clip(0, 7)
    base_ang = rng.uniform(npts, 0, 360)
    node_ids = (1000 + 37 * np.arange(max(n_nodes, 1))).astype(np.int32)
    base_node = rng.integers(npts, 0, max(n_nodes, 1))
    if descriptor_families:
        fam, members, spread = [int(v) for v in descriptor_families]
        frng = synth.Rng(int(seed) * 7919 + 104729)
        fam = min(fam, npts // max(members, 1))
        fam_desc = frng.integers(fam * 32, 0, 256).astype(np.uint8).reshape(fam, 32)
        fam_node = frng.integers(fam, 0, max(n_nodes, 1))
        for f in range(fam):
            for j in range(members):
                base_desc[f * members + j] = synth._flip(frng, fam_desc[f], spread)
                base_node[f * members + j] = fam_node[f]
    out = []
    for i in range(n_kf):
        ni = sizes[i]
        back = step[i] if np.ndim(step) else step * i
        C = np.array([0.0, 0.0, -float(back)]) + (rng.uniform(3, -0.08, 0.08) if i else np.zeros(3))
        R = synth._so3_exp(np.radians(rng.uniform(3, -1.0, 1.0))) if i else np.eye(3)
        R32 = R.astype(F32)
        ow = C.astype(F32)
        t32 = (-(R32.astype(np.float64) @ ow.astype(np.float64))).astype(F32)
        Xc = (P - C) @ R.T
        u = fx * Xc[:, 0] / Xc[:, 2] + cx + rng.normal(npts) * noise
        v = fy * Xc[:, 1] / Xc[:, 2] + cy + rng.normal(npts) * noise
        seen = (Xc[:, 2] > 1.0) & (u > 10) & (u < w - 10) & (v > 10) & (v < h - 10) & (rng.uniform(npts) < p_seen)
        ids = np.nonzero(seen)[0]
        ids = ids[np.argsort(rng.uniform(len(ids)), kind="stable")][:ni]
        m = len(ids)
        x = np.concatenate([u[ids], rng.uniform(ni - m, 10, w - 10)]).astype(F32)
        y = np.concatenate([v[ids], rng.uniform(ni - m, 10, h - 10)]).astype(F32)
        z = np.concatenate([Xc[ids, 2] * (1.0 + rng.normal(m) * 0.01), rng.uniform(ni - m, 5.0, 45.0)])
        stereo = (z < stereo_depth) & (rng.uniform(ni) < p_stereo)
        depth = np.where(stereo, z, -1.0).astype(F32)
        ur = np.where(stereo, x.astype(np.float64) - KITTI_BF / np.where(stereo, depth, 1.0).astype(np.float64), -1.0).astype(F32)
        octave = np.concatenate([np.clip(base_oct[ids] + rng.integers(m, -1, 2), 0, 7), rng.integers(ni - m, 0, 8)]).astype(np.int32)
        rot = 8.0 * i + rng.normal(m) * np.where(rng.uniform(m) < 0.9, 2.0, 80.0)
        angle = np.concatenate([(base_ang[ids] + rot) % 360.0, rng.uniform(ni - m, 0, 360)]).astype(F32)
        angle[angle >= 360.0] = 0.0
        desc = np.concatenate([np.stack([synth._flip(rng, base_desc[j], flip_bits) for j in ids]) if m else np.zeros((0, 32), np.uint8),
                               rng.integers((ni - m) * 32, 0, 256).astype(np.uint8).reshape(-1, 32)])
        node = np.concatenate([base_node[ids], rng.integers(ni - m, 0, max(n_nodes, 1))])
        wrong = rng.uniform(ni) < p_wrong
        node = np.where(wrong, rng.integers(ni, 0, max(n_nodes, 1)), node)
        node = np.where(rng.uniform(ni) < p_none, -1, node_ids[node]).astype(np.int32)
        occupied = (rng.uniform(ni) < p_occupied).astype(np.uint8)
        order = np.argsort(rng.uniform(ni), kind="stable")     # the keyframe's own feature order
        kf = {"x": x[order], "y": y[order], "octave": octave[order], "angle": angle[order], "u_right": ur[order], "depth": depth[order],
              "desc": np.ascontiguousarray(desc[order]), "node": node[order], "occupied": occupied[order],
              "point": np.concatenate([ids, np.full(ni - m, -1)])[order].astype(np.int64),
              "R": R32, "t": t32, "ow": ow,
              "K8": (F32(fx), F32(fy), F32(cx), F32(cy), F32(1.0) / F32(fx), F32(1.0) / F32(fy), F32(KITTI_BF) / F32(fx), F32(KITTI_BF)),
              "scale_factors": sig, "level_sigma2": (sig * sig).astype(F32)}
        if raw_shift:
            kf["x_raw"] = (kf["x"] + F32(raw_shift)).astype(F32); kf["y_raw"] = (kf["y"] - F32(raw_shift)).astype(F32)
        out.append(kf)
    return out


def tri_problem(seed, k=3, n1=300, n2=300, only_stereo=0, check_orientation=1, triangulate=1, chain=1, **kw):
    """One CreateNewMapPoints problem: keyframe_set(seed, k + 1) with n1 features in the current keyframe and n2 in each neighbour."""
    kfs = keyframe_set(seed, n_kf=k + 1, sizes=[n1] + [n2] * k, **kw)
    return problem_of(kfs, only_stereo, check_orientation, triangulate, chain)


def problem_of(kfs, only_stereo=0, check_orientation=1, triangulate=1, chain=1):
    f12 = np.stack([compute_f12(kfs[0], kf) for kf in kfs[1:]]) if len(kfs) > 1 else np.zeros((0, 3, 3), F32)
    return {"kf1": kfs[0], "kf2": kfs[1:], "f12": f12, "only_stereo": only_stereo, "check_orientation": check_orientation,
            "triangulate": triangulate, "chain": chain, "ratio_factor": F32(1.5) * F32(1.2)}


def bow_pair(seed, na=300, nb=300, n_nodes=12, families=(40, 6, 8), flip_bits=8, p_point=0.8, **kw):
    """Two views of one scene as the sides of ORBmatcher::SearchByBoW (ps_bow_side): the keyframe dicts of keyframe_set with
    has_point (= occupied, drawn with p_point) added; "point" is the world point behind a feature, -1 for clutter.  Side a is
    pKF / pKF1, side b is F / pKF2."""
    kfs = keyframe_set(seed, n_kf=2, sizes=[na, nb], n_nodes=n_nodes, flip_bits=flip_bits, p_occupied=p_point, descriptor_families=families, **kw)
    return tuple(dict(kf, has_point=kf["occupied"]) for kf in kfs)
