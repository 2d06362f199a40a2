"""Host-side mirror of the hot members of ORB_SLAM2::ORBmatcher (/root/reference/include/ORBmatcher.h:47-118)
on top of the C-ABI.  The reference writes MapPoint pointers into the Frame; here the same assignments come
back as index arrays (index of the source point, -1 for NULL)."""
import ctypes

import numpy as np

from ._lib import lib, check


class _BfProblem(ctypes.Structure):
    _fields_ = [("q_desc", ctypes.c_void_p), ("q_angle", ctypes.c_void_p), ("q_valid", ctypes.c_void_p),
                ("nq", ctypes.c_int32), ("t_desc", ctypes.c_void_p), ("t_angle", ctypes.c_void_p),
                ("nt", ctypes.c_int32), ("query_of_train", ctypes.c_void_p), ("nmatches", ctypes.c_int32)]


lib.ps_matcher_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
lib.ps_matcher_destroy.argtypes = [ctypes.c_void_p]
lib.ps_matcher_destroy.restype = None
lib.ps_hamming_matrix.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                  ctypes.c_void_p]
lib.ps_match_bruteforce.argtypes = [ctypes.c_void_p, ctypes.POINTER(_BfProblem), ctypes.c_int, ctypes.c_float,
                                    ctypes.c_int]


lib.ps_matcher_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
lib.ps_distinctive_descriptors.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]


class ORBmatcher:
    TH_HIGH = 100
    TH_LOW = 50
    TH_HIGH_FORDYNAMIC = 130
    RADIUS_FORDYNAMIC = 5
    HISTO_LENGTH = 30

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        self._h = ctypes.c_void_p()
        check(lib.ps_matcher_create(device, ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib.ps_matcher_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_kernel_ms(self):
        v = ctypes.c_float(0)
        check(lib.ps_matcher_last_kernel_ms(self._h, ctypes.byref(v)))
        return v.value

    def DescriptorDistanceMatrix(self, q, t):
        """bulk ORBmatcher::DescriptorDistance: uint16 [nq, nt]"""
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        out = np.zeros((len(q), len(t)), np.uint16)
        check(lib.ps_hamming_matrix(self._h, q.ctypes.data, len(q), t.ctypes.data, len(t), out.ctypes.data))
        return out

    def ComputeDistinctiveDescriptors(self, desc_lists):
        """desc_lists: one uint8 [n_i, 32] array per map point (its observations).  Returns int32 best index per point."""
        n = len(desc_lists)
        off = np.zeros(n + 1, np.int32)
        for i, d in enumerate(desc_lists):
            off[i + 1] = off[i] + len(d)
        cat = np.ascontiguousarray(np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in desc_lists] + [np.zeros((1, 32), np.uint8)]))
        best = np.zeros(n, np.int32)
        check(lib.ps_distinctive_descriptors(self._h, cat.ctypes.data, off.ctypes.data, n, best.ctypes.data))
        return best

    def SearchByBruceMatching(self, problems):
        """problems: list of dicts {q_desc [nq,32], q_angle [nq], q_valid [nq], t_desc [nt,32], t_angle [nt]}
        (one per tracked object).  Returns a list of (nmatches, query_of_train int32[nt])."""
        n = len(problems)
        arr = (_BfProblem * n)()
        keep = []
        for i, p in enumerate(problems):
            qd = np.ascontiguousarray(p["q_desc"], np.uint8).reshape(-1, 32)
            td = np.ascontiguousarray(p["t_desc"], np.uint8).reshape(-1, 32)
            qa = np.ascontiguousarray(p["q_angle"], np.float32)
            ta = np.ascontiguousarray(p["t_angle"], np.float32)
            qv = np.ascontiguousarray(p["q_valid"], np.uint8)
            out = np.full(max(len(td), 1), -1, np.int32)
            keep.append((qd, td, qa, ta, qv, out))
            arr[i] = _BfProblem(qd.ctypes.data, qa.ctypes.data, qv.ctypes.data, len(qd), td.ctypes.data,
                                ta.ctypes.data, len(td), out.ctypes.data, 0)
        check(lib.ps_match_bruteforce(self._h, arr, n, self.mfNNratio, 1 if self.mbCheckOrientation else 0))
        return [(arr[i].nmatches, keep[i][5][:len(keep[i][1])].copy()) for i in range(n)]


# ---- windowed matching (the three SearchByProjection overloads) ---------------------------------------------
FRAME_GRID_COLS, FRAME_GRID_ROWS = 64, 48      # /root/reference/include/Frame.h:40-41


def build_grid(x, y, min_x, min_y, gw_inv, gh_inv):
    """Frame::AssignFeaturesToGrid / PosInGrid (/root/reference/src/Frame.cc:1636-1656, 2027-2037) as CSR:
    returns (cell_off int32[64*48+1], cell_idx int32[<=n]) with cell = ix * 48 + iy, insertion order inside a cell."""
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32)
    fx = (x - np.float32(min_x)) * np.float32(gw_inv); fy = (y - np.float32(min_y)) * np.float32(gh_inv)
    px = np.where(fx >= 0, np.floor(fx + np.float32(0.5)), np.ceil(fx - np.float32(0.5))).astype(np.int64)   # C round()
    py = np.where(fy >= 0, np.floor(fy + np.float32(0.5)), np.ceil(fy - np.float32(0.5))).astype(np.int64)
    ok = (px >= 0) & (px < FRAME_GRID_COLS) & (py >= 0) & (py < FRAME_GRID_ROWS)
    cell = px * FRAME_GRID_ROWS + py
    idx = np.nonzero(ok)[0]
    order = np.argsort(cell[idx], kind="stable")
    cell_idx = idx[order].astype(np.int32)
    counts = np.bincount(cell[idx], minlength=FRAME_GRID_COLS * FRAME_GRID_ROWS)
    cell_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return cell_off, cell_idx


class _ProjTrain(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("octave", ctypes.c_void_p),
                ("angle", ctypes.c_void_p), ("u_right", ctypes.c_void_p), ("desc", ctypes.c_void_p),
                ("occupied", ctypes.c_void_p), ("in_bbox", ctypes.c_void_p), ("cell_off", ctypes.c_void_p),
                ("cell_idx", ctypes.c_void_p), ("min_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("grid_w_inv", ctypes.c_float), ("grid_h_inv", ctypes.c_float)]


class _ProjProblem(ctypes.Structure):
    _fields_ = [("train", _ProjTrain), ("nq", ctypes.c_int32), ("q_valid", ctypes.c_void_p), ("q_desc", ctypes.c_void_p),
                ("q_observed", ctypes.c_void_p), ("q_angle", ctypes.c_void_p), ("q_u", ctypes.c_void_p),
                ("q_v", ctypes.c_void_p), ("q_ur", ctypes.c_void_p), ("q_radius", ctypes.c_void_p),
                ("q_radius_er", ctypes.c_void_p), ("q_min_level", ctypes.c_void_p), ("q_max_level", ctypes.c_void_p),
                ("q_xw", ctypes.c_void_p), ("q_octave", ctypes.c_void_p), ("frame_mode", ctypes.c_int32),
                ("mono", ctypes.c_int32), ("tcw", ctypes.c_float * 16), ("tlw", ctypes.c_float * 16),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("mbf", ctypes.c_float), ("mb", ctypes.c_float), ("bounds", ctypes.c_float * 4),
                ("scale_factors", ctypes.c_float * 8), ("th", ctypes.c_float), ("th_dist", ctypes.c_int32),
                ("ratio_test", ctypes.c_int32), ("nn_ratio", ctypes.c_float), ("check_orientation", ctypes.c_int32),
                ("use_bbox", ctypes.c_int32), ("match_of_train", ctypes.c_void_p), ("nmatches", ctypes.c_int32)]


lib.ps_search_by_projection.argtypes = [ctypes.c_void_p, ctypes.POINTER(_ProjProblem), ctypes.c_int]


def _arr(a, dt):
    return np.ascontiguousarray(a, dt)


def _frame_handles(problems):
    """(ctypes array of ps_frame* or None per problem) when any problem of the batch is frame-backed, else None"""
    fr = [pr["train"].get("frame") for pr in problems]
    if all(f is None for f in fr):
        return None
    return (ctypes.c_void_p * len(fr))(*[None if f is None else f._h.value for f in fr])


def _fill_train(t, F, keep, *, need=("angle", "u_right", "occupied", "in_bbox")):
    """One ps_proj_train from a searched-side dict: x, y, octave, desc, cell_off, cell_idx, grid and, of angle, u_right, occupied and
    in_bbox, those the call reads (`need`; angle and occupied default to zeros, in_bbox to ones) - or "frame" = a DeviceFrame that
    holds the keypoints and the grid, beside which only occupied and in_bbox stay host arrays.  Returns the number of keypoints."""
    frame = F.get("frame")
    if frame is None:
        n = len(F["x"])
        a = dict(x=_arr(F["x"], np.float32), y=_arr(F["y"], np.float32), octave=_arr(F["octave"], np.int32),
                 desc=_arr(F["desc"], np.uint8).reshape(-1, 32), cell_off=_arr(F["cell_off"], np.int32), cell_idx=_arr(F["cell_idx"], np.int32))
        t.min_x, t.min_y, t.grid_w_inv, t.grid_h_inv = [float(v) for v in F["grid"]]
    else:
        n, a = len(frame), {}
    for k in need:
        if k == "u_right" or k == "angle":                  # in the frame's slab, when there is one
            if frame is None:
                a[k] = np.zeros(n, np.float32) if k == "angle" and k not in F else _arr(F[k], np.float32)
        else:
            a[k] = _arr(F[k], np.uint8) if k in F else np.full(n, k == "in_bbox", np.uint8)
    for k, v in a.items():
        if len(v) != n and k != "cell_off" and k != "cell_idx":
            raise ValueError("the arrays of a searched side differ in length: %s has %d entries, the side %d keypoints" % (k, len(v), n))
        setattr(t, k, v.ctypes.data)
    keep.append(a)
    t.n = n
    return n


def _prepare_projection(self, problems):
    """the ps_proj_problem array of a batch: (array, frame handles or None, buffers to keep alive, outputs)"""
    n = len(problems)
    arr = (_ProjProblem * n)()
    keep, outs = [], []
    for i, pr in enumerate(problems):
        _fill_projection_problem(self, arr[i], pr, keep, outs)
    return arr, _frame_handles(problems), keep, outs


def _search_by_projection(self, problems, partial_ok=False):
    """problems: list of dicts, see SearchByProjectionFrame / SearchByProjectionPoints for the two layouts.  A problem whose
    train dict has "frame" = a DeviceFrame (pointslot_amd.frame) takes its train side from that handle and needs only "occupied"
    (and "in_bbox") beside it.  partial_ok: when a
    problem overflows even the wide candidate store the call fails with PS_ERR_CAPACITY after serving all the others; with
    partial_ok the results come back anyway, nmatches = -1 marking the problems that failed."""
    n = len(problems)
    arr, frames, keep, outs = _prepare_projection(self, problems)
    if frames is None:
        rc = lib.ps_search_by_projection(self._h, arr, n)
    else:
        lib.ps_search_by_projection_frames.argtypes = [ctypes.c_void_p, ctypes.POINTER(_ProjProblem), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
        rc = lib.ps_search_by_projection_frames(self._h, arr, frames, n)
    if not (partial_ok and rc == -3):
        check(rc)
    return [(arr[i].nmatches, outs[i][0][:outs[i][1]].copy()) for i in range(n)]


def _fill_projection_problem(self, p, pr, keep, outs):
    """one ps_proj_problem from its dict (see _search_by_projection)"""
    nt = _fill_train(p.train, pr["train"], keep)
    q = pr["query"]
    nq = len(q["valid"])
    a = dict(q_valid=_arr(q["valid"], np.uint8), q_desc=_arr(q["desc"], np.uint8).reshape(-1, 32),
             q_observed=_arr(q["observed"], np.uint8))
    p.frame_mode = 1 if pr["mode"] == "frame" else 0
    if p.frame_mode:
        a.update(q_angle=_arr(q["angle"], np.float32), q_xw=_arr(q["xw"], np.float32), q_octave=_arr(q["octave"], np.int32))
        p.tcw = (ctypes.c_float * 16)(*np.asarray(pr["tcw"], np.float32).reshape(16))
        p.tlw = (ctypes.c_float * 16)(*np.asarray(pr["tlw"], np.float32).reshape(16))
        p.fx, p.fy, p.cx, p.cy, p.mbf, p.mb = [float(v) for v in pr["K6"]]
        p.bounds = (ctypes.c_float * 4)(*[float(v) for v in pr["bounds"]])
        p.th = float(pr["th"]); p.mono = 1 if pr.get("mono") else 0
        p.th_dist = ORBmatcher.TH_HIGH; p.ratio_test = 0; p.nn_ratio = self.mfNNratio
        p.check_orientation = 1 if self.mbCheckOrientation else 0; p.use_bbox = 0
    else:
        obj = bool(pr.get("object"))
        th = np.float32(pr["th"])
        lvl = np.asarray(q["level"], np.int32)
        sf = np.asarray(pr["scale_factors"], np.float32)
        r = np.where(np.asarray(q["view_cos"], np.float32) > np.float32(0.998), np.float32(2.5), np.float32(4.0)).astype(np.float32)
        if float(th) != 1.0:
            r = (r * th).astype(np.float32)
        rer = (r * sf[lvl]).astype(np.float32)
        a.update(q_u=_arr(q["proj_x"], np.float32), q_v=_arr(q["proj_y"], np.float32), q_ur=_arr(q["proj_xr"], np.float32),
                 q_radius=np.full(nq, 5.0, np.float32) if obj else rer, q_radius_er=rer,
                 q_min_level=(lvl - 1).astype(np.int32), q_max_level=(lvl + 1 if obj else lvl).astype(np.int32))
        p.th_dist = ORBmatcher.TH_HIGH_FORDYNAMIC if obj else ORBmatcher.TH_HIGH
        p.ratio_test = 1; p.nn_ratio = self.mfNNratio; p.check_orientation = 0; p.use_bbox = 1 if obj else 0
    p.scale_factors = (ctypes.c_float * 8)(*np.asarray(pr["scale_factors"], np.float32))
    p.nq = nq
    for k, v in a.items():
        setattr(p, k, v.ctypes.data)
    out = np.full(max(nt, 1), -1, np.int32)
    p.match_of_train = out.ctypes.data
    keep.append(a); outs.append((out, nt))


ORBmatcher.SearchByProjection = _search_by_projection
ORBmatcher._prepare_projection = _prepare_projection


class _FuseProblem(ctypes.Structure):
    _fields_ = [("train", _ProjTrain), ("nq", ctypes.c_int32), ("q_valid", ctypes.c_void_p), ("q_pos", ctypes.c_void_p),
                ("q_normal", ctypes.c_void_p), ("q_min_dist", ctypes.c_void_p), ("q_max_dist", ctypes.c_void_p), ("q_desc", ctypes.c_void_p),
                ("rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("ow", ctypes.c_float * 3),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("bf", ctypes.c_float),
                ("bounds", ctypes.c_double * 4), ("scale_factors", ctypes.c_float * 8), ("inv_level_sigma2", ctypes.c_float * 8),
                ("log_scale_factor", ctypes.c_float), ("n_levels", ctypes.c_int32), ("th", ctypes.c_float),
                ("best_idx", ctypes.c_void_p), ("best_dist", ctypes.c_void_p)]


lib.ps_fuse_search.argtypes = [ctypes.c_void_p, ctypes.POINTER(_FuseProblem), ctypes.c_int]


def _fuse_search(self, problems):
    """The search half of ORBmatcher::Fuse (KeyFrame / ObjectKeyFrame variants).  problems: list of dicts
    {train (keyframe features + grid, as for SearchByProjection), query {valid, pos [m,3], normal [m,3], min_dist, max_dist, desc},
     R 3x3, t 3, ow 3, K5 (fx, fy, cx, cy, bf), bounds (minX, maxX, minY, maxY), scale_factors, inv_level_sigma2,
     log_scale_factor, n_levels, th}.  Returns a list of (best_idx int32[m], best_dist int32[m])."""
    n = len(problems)
    arr = (_FuseProblem * n)()
    keep, outs = [], []
    for i, pr in enumerate(problems):
        p = arr[i]
        _fill_train(p.train, pr["train"], keep, need=("u_right",))
        q = pr["query"]
        m = len(q["valid"])
        a = dict(q_valid=_arr(q["valid"], np.uint8), q_pos=_arr(q["pos"], np.float32).reshape(-1, 3), q_normal=_arr(q["normal"], np.float32).reshape(-1, 3),
                 q_min_dist=_arr(q["min_dist"], np.float32), q_max_dist=_arr(q["max_dist"], np.float32), q_desc=_arr(q["desc"], np.uint8).reshape(-1, 32))
        for k, v in a.items():
            setattr(p, k, v.ctypes.data)
        p.nq = m
        p.rcw = (ctypes.c_float * 9)(*np.asarray(pr["R"], np.float32).reshape(9))
        p.tcw = (ctypes.c_float * 3)(*np.asarray(pr["t"], np.float32).reshape(3))
        p.ow = (ctypes.c_float * 3)(*np.asarray(pr["ow"], np.float32).reshape(3))
        p.fx, p.fy, p.cx, p.cy, p.bf = [float(v) for v in pr["K5"]]
        p.bounds = (ctypes.c_double * 4)(*[float(v) for v in pr["bounds"]])
        p.scale_factors = (ctypes.c_float * 8)(*np.asarray(pr["scale_factors"], np.float32))
        p.inv_level_sigma2 = (ctypes.c_float * 8)(*np.asarray(pr["inv_level_sigma2"], np.float32))
        p.log_scale_factor = float(pr["log_scale_factor"]); p.n_levels = int(pr["n_levels"]); p.th = float(pr["th"])
        bi = np.full(max(m, 1), -1, np.int32); bd = np.full(max(m, 1), 256, np.int32)
        p.best_idx = bi.ctypes.data; p.best_dist = bd.ctypes.data
        keep.append(a); outs.append((bi, bd, m))
    frames = _frame_handles(problems)
    if frames is None:
        check(lib.ps_fuse_search(self._h, arr, n))
    else:
        lib.ps_fuse_search_frames.argtypes = [ctypes.c_void_p, ctypes.POINTER(_FuseProblem), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
        check(lib.ps_fuse_search_frames(self._h, arr, frames, n))
    return [(bi[:m].copy(), bd[:m].copy()) for bi, bd, m in outs]


ORBmatcher.FuseSearch = _fuse_search


# ---- LocalMapping::CreateNewMapPoints: SearchForTriangulation + triangulation (ps_create_new_map_points) ----------------
class _TriKeyframe(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("x_raw", ctypes.c_void_p), ("y_raw", ctypes.c_void_p),
                ("octave", ctypes.c_void_p), ("angle", ctypes.c_void_p), ("u_right", ctypes.c_void_p), ("depth", ctypes.c_void_p),
                ("desc", ctypes.c_void_p), ("node", ctypes.c_void_p), ("occupied", ctypes.c_void_p),
                ("rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("ow", ctypes.c_float * 3),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("invfx", ctypes.c_float), ("invfy", ctypes.c_float), ("mb", ctypes.c_float), ("mbf", ctypes.c_float),
                ("scale_factors", ctypes.c_float * 8), ("level_sigma2", ctypes.c_float * 8)]


class _TriProblem(ctypes.Structure):
    _fields_ = [("kf1", _TriKeyframe), ("k", ctypes.c_int32), ("kf2", ctypes.POINTER(_TriKeyframe)), ("f12", ctypes.c_void_p),
                ("only_stereo", ctypes.c_int32), ("check_orientation", ctypes.c_int32), ("triangulate", ctypes.c_int32),
                ("chain", ctypes.c_int32), ("ratio_factor", ctypes.c_float), ("match", ctypes.c_void_p), ("nmatches", ctypes.c_void_p),
                ("x3d", ctypes.c_void_p), ("status", ctypes.c_void_p), ("nnew", ctypes.c_void_p)]


TRI_STATUS = ("created", "no match", "slot occupied", "low parallax", "w == 0", "z1 <= 0", "z2 <= 0", "reprojection 1", "reprojection 2",
              "zero distance", "scale ratio", "neighbour skipped")
_TRI_KEYS = (("x", np.float32), ("y", np.float32), ("octave", np.int32), ("angle", np.float32), ("u_right", np.float32))


def _fill_tri_keyframe(c, kf, keep, frame=None):
    """one ps_tri_keyframe from a keyframe dict: x, y, octave, angle, u_right, depth, desc, node, occupied (x_raw, y_raw optional),
    R (GetRotation), t (GetTranslation), ow (GetCameraCenter), K8 = (fx, fy, cx, cy, invfx, invfy, mb, mbf), scale_factors, level_sigma2.
    frame: the DeviceFrame that holds x .. desc (keyframe 1 only); the dict then needs only n-sized depth, node, occupied."""
    a = dict(depth=_arr(kf["depth"], np.float32), node=_arr(kf["node"], np.int32), occupied=_arr(kf["occupied"], np.uint8))
    n = len(a["node"])
    if frame is None:
        a.update({k: _arr(kf[k], dt) for k, dt in _TRI_KEYS})
        a["desc"] = _arr(kf["desc"], np.uint8).reshape(-1, 32)
    if kf.get("x_raw") is not None:
        a.update(x_raw=_arr(kf["x_raw"], np.float32), y_raw=_arr(kf["y_raw"], np.float32))
    if any(len(v) != n for v in a.values()):
        raise ValueError("the arrays of a keyframe differ in length")
    keep.append(a)
    c.n = n
    for k, v in a.items():
        setattr(c, k, v.ctypes.data)
    c.rcw = (ctypes.c_float * 9)(*np.asarray(kf["R"], np.float32).reshape(9))
    c.tcw = (ctypes.c_float * 3)(*np.asarray(kf["t"], np.float32).reshape(3))
    c.ow = (ctypes.c_float * 3)(*np.asarray(kf["ow"], np.float32).reshape(3))
    c.fx, c.fy, c.cx, c.cy, c.invfx, c.invfy, c.mb, c.mbf = [float(v) for v in kf["K8"]]
    c.scale_factors = (ctypes.c_float * 8)(*np.asarray(kf["scale_factors"], np.float32))
    c.level_sigma2 = (ctypes.c_float * 8)(*np.asarray(kf["level_sigma2"], np.float32))
    return n


lib.ps_create_new_map_points.argtypes = [ctypes.c_void_p, ctypes.POINTER(_TriProblem), ctypes.c_int]
lib.ps_create_new_map_points_frames.argtypes = [ctypes.c_void_p, ctypes.POINTER(_TriProblem), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]


def _create_new_map_points(self, problems, partial_ok=False):
    """LocalMapping::CreateNewMapPoints for a batch of keyframes.  problems: list of dicts {kf1, kf2: [neighbours in order],
    f12: [k, 3, 3] ComputeF12(kf1, kf2[i]), only_stereo, check_orientation (default: the matcher's), triangulate (default 1),
    chain (default 1), ratio_factor (1.5f * mfScaleFactor)}; keyframe dicts as in _fill_tri_keyframe, and kf1 may carry
    "frame" = a DeviceFrame holding its keys and descriptors.  Returns per problem a dict: match int32 [k, n1] (idx2 or -1),
    nmatches int32 [k], status uint8 [k, n1] and x3d float32 [k, n1, 3] (triangulate), nnew; "failed" = True for a problem beyond
    the limits when partial_ok lets the call return after PS_ERR_CAPACITY."""
    n = len(problems)
    arr = (_TriProblem * n)()
    keep, outs, frames = [], [], []
    for i, pr in enumerate(problems):
        p = arr[i]
        fr = pr["kf1"].get("frame")
        frames.append(fr)
        n1 = _fill_tri_keyframe(p.kf1, pr["kf1"], keep, fr)
        k = len(pr["kf2"])
        nb = (_TriKeyframe * max(k, 1))()
        for j, kf in enumerate(pr["kf2"]):
            _fill_tri_keyframe(nb[j], kf, keep)
        f12 = _arr(pr["f12"], np.float32).reshape(-1, 9) if k else np.zeros((1, 9), np.float32)
        if len(f12) != max(k, 1):
            raise ValueError("one F12 per neighbour")
        p.k = k; p.kf2 = nb; p.f12 = f12.ctypes.data
        p.only_stereo = 1 if pr.get("only_stereo") else 0
        p.check_orientation = 1 if pr.get("check_orientation", self.mbCheckOrientation) else 0
        p.triangulate = 1 if pr.get("triangulate", 1) else 0
        p.chain = 1 if pr.get("chain", 1) else 0
        p.ratio_factor = float(pr.get("ratio_factor", np.float32(1.5) * np.float32(1.2)))
        o = dict(match=np.full((max(k, 1), max(n1, 1)), -1, np.int32), nmatches=np.zeros(max(k, 1), np.int32),
                 x3d=np.zeros((max(k, 1), max(n1, 1), 3), np.float32), status=np.full((max(k, 1), max(n1, 1)), 255, np.uint8),
                 nnew=np.full(1, -1, np.int32))
        for name, v in o.items():
            setattr(p, name, v.ctypes.data)
        keep.append((nb, f12)); outs.append((o, k, n1, p.triangulate))
    if all(f is None for f in frames):
        rc = lib.ps_create_new_map_points(self._h, arr, n)
    else:
        handles = (ctypes.c_void_p * n)(*[None if f is None else f._h.value for f in frames])
        rc = lib.ps_create_new_map_points_frames(self._h, arr, handles, n)
    if not (partial_ok and rc == -3):
        check(rc)
    res = []
    for o, k, n1, tri in outs:
        r = dict(match=o["match"][:k, :n1].copy(), nmatches=o["nmatches"][:k].copy(), nnew=int(o["nnew"][0]), failed=int(o["nnew"][0]) < 0)
        if tri:
            r.update(status=o["status"][:k, :n1].copy(), x3d=o["x3d"][:k, :n1].copy())
        res.append(r)
    return res


def _search_for_triangulation(self, kf1, kf2, F12, only_stereo):
    """ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo): (nmatches, [(idx1, idx2), ...])."""
    r = _create_new_map_points(self, [dict(kf1=kf1, kf2=[kf2], f12=np.asarray(F12, np.float32).reshape(1, 9), only_stereo=only_stereo,
                                           triangulate=0, chain=0)])[0]
    m = r["match"][0]
    return int(r["nmatches"][0]), [(int(i), int(m[i])) for i in np.nonzero(m >= 0)[0]]


ORBmatcher.CreateNewMapPoints = _create_new_map_points
ORBmatcher.SearchForTriangulation = _search_for_triangulation


# ---- ORBmatcher::SearchByBoW, both overloads (ps_search_by_bow) ------------------------------------------------------------
class _BowSide(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("desc", ctypes.c_void_p), ("angle", ctypes.c_void_p), ("node", ctypes.c_void_p),
                ("has_point", ctypes.c_void_p)]


class _BowSearchProblem(ctypes.Structure):
    _fields_ = [("a", _BowSide), ("b", _BowSide), ("mode", ctypes.c_int32), ("nn_ratio", ctypes.c_float),
                ("check_orientation", ctypes.c_int32), ("match", ctypes.c_void_p), ("nmatches", ctypes.c_int32)]


lib.ps_search_by_bow.argtypes = [ctypes.c_void_p, ctypes.POINTER(_BowSearchProblem), ctypes.c_int]


def _fill_bow_side(c, side, keep, need_points):
    """one ps_bow_side from a dict: desc [n, 32], angle [n], node [n] (ps_bow_transform's node[]), has_point [n] (optional on the
    Frame side of mode 0)"""
    a = dict(desc=_arr(side["desc"], np.uint8).reshape(-1, 32), angle=_arr(side["angle"], np.float32), node=_arr(side["node"], np.int32))
    if need_points or side.get("has_point") is not None:
        a["has_point"] = _arr(side["has_point"], np.uint8)
    n = len(a["node"])
    if any(len(v) != n for v in a.values()):
        raise ValueError("the arrays of a side differ in length")
    keep.append(a)
    c.n = n
    for k, v in a.items():
        setattr(c, k, v.ctypes.data)
    return n


def _search_by_bow(self, problems, partial_ok=False):
    """ORBmatcher::SearchByBoW for a batch.  problems: list of dicts {a, b: sides as in _fill_bow_side, mode: 0 (KeyFrame*, Frame&)
    or 1 (KeyFrame*, KeyFrame*), nn_ratio and check_orientation (default: the matcher's)}.  Returns per problem
    (nmatches, match int32): mode 0 [b.n] holding indices into a, mode 1 [a.n] holding indices into b, -1 = NULL; nmatches = -1
    for a problem beyond the limits when partial_ok lets the call return after PS_ERR_CAPACITY."""
    n = len(problems)
    if n == 0:
        return []
    arr = (_BowSearchProblem * n)()
    keep, outs = [], []
    for i, pr in enumerate(problems):
        p = arr[i]
        p.mode = int(pr.get("mode", 0))
        na = _fill_bow_side(p.a, pr["a"], keep, True)
        nb = _fill_bow_side(p.b, pr["b"], keep, p.mode == 1)
        p.nn_ratio = float(pr.get("nn_ratio", self.mfNNratio))
        p.check_orientation = 1 if pr.get("check_orientation", self.mbCheckOrientation) else 0
        m = nb if p.mode == 0 else na
        out = np.full(max(m, 1), -3, np.int32)
        p.match = out.ctypes.data; p.nmatches = -2
        outs.append((out, m))
    rc = lib.ps_search_by_bow(self._h, arr, n)
    if not (partial_ok and rc == -3):
        check(rc)
    return [(int(arr[i].nmatches), outs[i][0][:outs[i][1]].copy()) for i in range(n)]


def _search_by_bow_one(self, a, b, mode=0):
    """SearchByBoW(pKF, F, vpMapPointMatches) (mode 0) / SearchByBoW(pKF1, pKF2, vpMatches12) (mode 1) for one pair"""
    return _search_by_bow(self, [dict(a=a, b=b, mode=mode)])[0]


ORBmatcher.SearchByBoWBatch = _search_by_bow
ORBmatcher.SearchByBoW = _search_by_bow_one


# ---- the loop-closure and relocalisation projection matchers (ps_kf_search, ps_search_by_sim3) ------------------------------
def _dot_double(a, b):
    """cv::Mat product convention of the repository: the float products and their sum in double, rounded to float once"""
    return np.float32(float(a[0]) * float(b[0]) + float(a[1]) * float(b[1]) + float(a[2]) * float(b[2]))


def decompose_scw(Scw):
    """The decomposition of a Sim3 pose at ORBmatcher.cc:422-426 / :1271-1275, as ONE stated model (cv::MatExpr division by a scalar
    is OpenCV-internal): the dot product of row 0 in double, scw = sqrt rounded to float, every entry of Rcw and tcw =
    float(double(entry) * (1.0 / double(scw))), Ow = -Rcw^T tcw with the products and their sum in double, rounded once.
    -> (Rcw float32 [3, 3], tcw float32 [3], Ow float32 [3], scw float32)"""
    S = np.asarray(Scw, np.float32).reshape(4, 4)
    r0 = S[0, :3]
    scw = np.float32(np.sqrt(float(r0[0]) * float(r0[0]) + float(r0[1]) * float(r0[1]) + float(r0[2]) * float(r0[2])))
    inv = 1.0 / float(scw)
    Rcw = (S[:3, :3].astype(np.float64) * inv).astype(np.float32)
    tcw = (S[:3, 3].astype(np.float64) * inv).astype(np.float32)
    Ow = np.array([np.float32(-float(_dot_double(Rcw[:, r], tcw))) for r in range(3)], np.float32)
    return Rcw, tcw, Ow, scw


def sim3_pair(s12, R12, t12):
    """sR12 = s12 * R12, sR21 = (1.0 / s12) * R12.t(), t21 = -sR21 * t12 (ORBmatcher.cc:1404-1406) as ONE stated model: every entry of
    sR12 = float(double(R12) * double(s12)), of sR21 = float(double(R12^T) * (1.0 / double(s12))), t21 with the products and their
    sum in double, negated, rounded once.  -> (sR12, t12, sR21, t21) as float32"""
    s = float(np.float32(s12))
    R = np.asarray(R12, np.float32).reshape(3, 3)
    t = np.asarray(t12, np.float32).reshape(3)
    sR12 = (R.astype(np.float64) * s).astype(np.float32)
    sR21 = (R.T.astype(np.float64) * (1.0 / s)).astype(np.float32)
    t21 = np.array([np.float32(-float(_dot_double(sR21[r], t))) for r in range(3)], np.float32)
    return sR12, t.copy(), sR21, t21


class _KfSearchProblem(ctypes.Structure):
    _fields_ = [("train", _ProjTrain), ("mode", ctypes.c_int32), ("nq", ctypes.c_int32), ("q_valid", ctypes.c_void_p), ("q_pos", ctypes.c_void_p),
                ("q_normal", ctypes.c_void_p), ("q_min_dist", ctypes.c_void_p), ("q_max_dist", ctypes.c_void_p), ("q_desc", ctypes.c_void_p),
                ("q_angle", ctypes.c_void_p), ("rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("ow", ctypes.c_float * 3),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("bounds", ctypes.c_float * 4),
                ("scale_factors", ctypes.c_float * 8), ("log_scale_factor", ctypes.c_float), ("n_levels", ctypes.c_int32), ("th", ctypes.c_float),
                ("th_dist", ctypes.c_int32), ("check_orientation", ctypes.c_int32), ("match_of_train", ctypes.c_void_p),
                ("best_idx", ctypes.c_void_p), ("best_dist", ctypes.c_void_p), ("nmatches", ctypes.c_int32)]


class _Sim3Side(ctypes.Structure):
    _fields_ = [("train", _ProjTrain), ("has_point", ctypes.c_void_p), ("pos", ctypes.c_void_p), ("min_dist", ctypes.c_void_p),
                ("max_dist", ctypes.c_void_p), ("point_desc", ctypes.c_void_p), ("already", ctypes.c_void_p),
                ("rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("bounds", ctypes.c_float * 4), ("scale_factors", ctypes.c_float * 8),
                ("log_scale_factor", ctypes.c_float), ("n_levels", ctypes.c_int32)]


class _Sim3Problem(ctypes.Structure):
    _fields_ = [("kf1", _Sim3Side), ("kf2", _Sim3Side), ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("sr12", ctypes.c_float * 9), ("t12", ctypes.c_float * 3), ("sr21", ctypes.c_float * 9), ("t21", ctypes.c_float * 3),
                ("th", ctypes.c_float), ("match12", ctypes.c_void_p), ("match1", ctypes.c_void_p), ("match2", ctypes.c_void_p),
                ("nfound", ctypes.c_int32)]


def _c_floats(v, n):
    return (ctypes.c_float * n)(*np.asarray(v, np.float32).reshape(n))


def _kf_search(self, problems, partial_ok=False, mode=None):
    """ps_kf_search for a batch.  problems: list of dicts {mode 0 / 1 / 2 (or the `mode` argument for all), train (see _fill_train),
    query {valid, pos [m, 3], normal [m, 3] (modes 0, 1), min_dist, max_dist, desc [m, 32], angle (mode 2)}, R, t, ow (decompose_scw
    for the Sim3 overloads; GetRotation / GetTranslation / GetCameraCenter of the frame in mode 2), K4 (fx, fy, cx, cy), bounds,
    scale_factors, log_scale_factor, n_levels, th, th_dist (mode 2: ORBdist), check_orientation (mode 2; default: the matcher's)}.
    Returns per problem a dict: nmatches, and match_of_train int32 [n] (modes 0, 2) or best_idx / best_dist int32 [m] (mode 1);
    nmatches = -1 marks a problem beyond the limits when partial_ok lets the call return after PS_ERR_CAPACITY."""
    n = len(problems)
    if n == 0:
        return []
    arr = (_KfSearchProblem * n)()
    keep, outs = [], []
    for i, pr in enumerate(problems):
        p = arr[i]
        p.mode = int(pr["mode"] if mode is None else mode)
        nt = _fill_train(p.train, pr["train"], keep, need=("angle", "occupied") if p.mode != 1 else ("angle",))
        q = pr["query"]
        m = len(q["valid"])
        a = dict(q_valid=_arr(q["valid"], np.uint8), q_pos=_arr(q["pos"], np.float32).reshape(-1, 3), q_min_dist=_arr(q["min_dist"], np.float32),
                 q_max_dist=_arr(q["max_dist"], np.float32), q_desc=_arr(q["desc"], np.uint8).reshape(-1, 32))
        if p.mode != 2:
            a["q_normal"] = _arr(q["normal"], np.float32).reshape(-1, 3)
        p.check_orientation = 1 if (p.mode == 2 and pr.get("check_orientation", self.mbCheckOrientation)) else 0
        if p.check_orientation:
            a["q_angle"] = _arr(q["angle"], np.float32)
        if any(len(v) != m for v in a.values()):
            raise ValueError("the arrays of a query side differ in length")
        for k, v in a.items():
            setattr(p, k, v.ctypes.data)
        p.nq = m
        p.rcw = _c_floats(pr["R"], 9); p.tcw = _c_floats(pr["t"], 3); p.ow = _c_floats(pr["ow"], 3)
        p.fx, p.fy, p.cx, p.cy = [float(v) for v in pr["K4"]]
        p.bounds = _c_floats(pr["bounds"], 4); p.scale_factors = _c_floats(pr["scale_factors"], 8)
        p.log_scale_factor = float(pr["log_scale_factor"]); p.n_levels = int(pr["n_levels"]); p.th = float(pr["th"])
        p.th_dist = int(pr.get("th_dist", ORBmatcher.TH_HIGH if p.mode == 2 else ORBmatcher.TH_LOW))
        o = dict(match_of_train=np.full(max(nt, 1), -3, np.int32), best_idx=np.full(max(m, 1), -3, np.int32), best_dist=np.full(max(m, 1), -3, np.int32))
        for name, v in o.items():
            setattr(p, name, v.ctypes.data)
        p.nmatches = -2
        keep.append(a); outs.append((o, nt, m, p.mode))
    fr = [pr["train"].get("frame") for pr in problems]
    if all(f is None for f in fr):
        rc = lib.ps_kf_search(self._h, arr, n)
    else:
        rc = lib.ps_kf_search_frames(self._h, arr, (ctypes.c_void_p * n)(*[None if f is None else f._h.value for f in fr]), n)
    if not (partial_ok and rc == -3):
        check(rc)
    res = []
    for i, (o, nt, m, md) in enumerate(outs):
        r = dict(nmatches=int(arr[i].nmatches))
        if md == 1:
            r.update(best_idx=o["best_idx"][:m].copy(), best_dist=o["best_dist"][:m].copy())
        else:
            r.update(match_of_train=o["match_of_train"][:nt].copy())
        res.append(r)
    return res


def _fill_sim3_side(c, kf, keep):
    """one ps_sim3_side from a keyframe dict: the searched-side keys of _fill_train plus has_point, pos [n, 3], min_dist, max_dist,
    point_desc [n, 32], already, R, t, bounds, scale_factors, log_scale_factor, n_levels"""
    n = _fill_train(c.train, kf, keep, need=("angle",))
    a = dict(has_point=_arr(kf["has_point"], np.uint8), pos=_arr(kf["pos"], np.float32).reshape(-1, 3), min_dist=_arr(kf["min_dist"], np.float32),
             max_dist=_arr(kf["max_dist"], np.float32), point_desc=_arr(kf["point_desc"], np.uint8).reshape(-1, 32),
             already=_arr(kf.get("already", np.zeros(n, np.uint8)), np.uint8))
    if any(len(v) != n for v in a.values()):
        raise ValueError("the arrays of a keyframe differ in length")
    keep.append(a)
    for k, v in a.items():
        setattr(c, k, v.ctypes.data)
    c.rcw = _c_floats(kf["R"], 9); c.tcw = _c_floats(kf["t"], 3); c.bounds = _c_floats(kf["bounds"], 4)
    c.scale_factors = _c_floats(kf["scale_factors"], 8)
    c.log_scale_factor = float(kf["log_scale_factor"]); c.n_levels = int(kf["n_levels"])
    return n


def _search_by_sim3_batch(self, problems, partial_ok=False):
    """ps_search_by_sim3 for a batch.  problems: list of dicts {kf1, kf2 (see _fill_sim3_side), K4 = keyframe 1's (fx, fy, cx, cy),
    s12, R12, t12 (through sim3_pair) or sr12, t12, sr21, t21 given outright, th}.  Returns per problem a dict: nfound, match12
    int32 [n1], match1 int32 [n1], match2 int32 [n2]; nfound = -1 marks a failed problem under partial_ok."""
    n = len(problems)
    if n == 0:
        return []
    arr = (_Sim3Problem * n)()
    keep, outs = [], []
    for i, pr in enumerate(problems):
        p = arr[i]
        n1 = _fill_sim3_side(p.kf1, pr["kf1"], keep)
        n2 = _fill_sim3_side(p.kf2, pr["kf2"], keep)
        p.fx, p.fy, p.cx, p.cy = [float(v) for v in pr["K4"]]
        sr12, t12, sr21, t21 = (pr["sr12"], pr["t12"], pr["sr21"], pr["t21"]) if "sr12" in pr else sim3_pair(pr["s12"], pr["R12"], pr["t12"])
        p.sr12 = _c_floats(sr12, 9); p.t12 = _c_floats(t12, 3); p.sr21 = _c_floats(sr21, 9); p.t21 = _c_floats(t21, 3)
        p.th = float(pr["th"])
        o = dict(match12=np.full(max(n1, 1), -3, np.int32), match1=np.full(max(n1, 1), -3, np.int32), match2=np.full(max(n2, 1), -3, np.int32))
        for name, v in o.items():
            setattr(p, name, v.ctypes.data)
        p.nfound = -2
        outs.append((o, n1, n2))
    f1 = [pr["kf1"].get("frame") for pr in problems]
    f2 = [pr["kf2"].get("frame") for pr in problems]
    if all(f is None for f in f1 + f2):
        rc = lib.ps_search_by_sim3(self._h, arr, n)
    else:
        h = lambda fs: (ctypes.c_void_p * n)(*[None if f is None else f._h.value for f in fs])
        rc = lib.ps_search_by_sim3_frames(self._h, arr, h(f1), h(f2), n)
    if not (partial_ok and rc == -3):
        check(rc)
    return [dict(nfound=int(arr[i].nfound), match12=o["match12"][:n1].copy(), match1=o["match1"][:n1].copy(), match2=o["match2"][:n2].copy())
            for i, (o, n1, n2) in enumerate(outs)]


def _search_by_sim3(self, *args, **kw):
    """SearchBySim3(problems) for a batch (see _search_by_sim3_batch), or the reference's own call for one pair:
    SearchBySim3(kf1, kf2, matches12, s12, R12, t12, th) with keyframe dicts as in _fill_sim3_side (K4 on kf1, `already` is built here)
    and matches12 int [n1] = the slot of keyframe 2 that holds vpMatches12[i] (GetIndexInKeyFrame), -1 for NULL, any other negative
    value for a point keyframe 2 does not hold.  -> (nfound, matches12 with the new pairs filled in)"""
    if len(args) == 1:
        return _search_by_sim3_batch(self, args[0], **kw)
    kf1, kf2, matches12, s12, R12, t12, th = args
    m12 = np.asarray(matches12, np.int64)
    n2 = len(kf2["has_point"])
    a1 = (m12 != -1).astype(np.uint8)
    a2 = np.zeros(n2, np.uint8)
    a2[m12[(m12 >= 0) & (m12 < n2)]] = 1
    r = _search_by_sim3_batch(self, [dict(kf1=dict(kf1, already=a1), kf2=dict(kf2, already=a2), K4=kf1["K4"], s12=s12, R12=R12, t12=t12, th=th)])[0]
    out = m12.copy()
    out[r["match12"] >= 0] = r["match12"][r["match12"] >= 0]
    return r["nfound"], out.astype(np.int32)


lib.ps_kf_search.argtypes = [ctypes.c_void_p, ctypes.POINTER(_KfSearchProblem), ctypes.c_int]
lib.ps_kf_search_frames.argtypes = [ctypes.c_void_p, ctypes.POINTER(_KfSearchProblem), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
lib.ps_search_by_sim3.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Sim3Problem), ctypes.c_int]
lib.ps_search_by_sim3_frames.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Sim3Problem), ctypes.POINTER(ctypes.c_void_p),
                                         ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]


def _kf_search_tuples(self, problems, mode, partial_ok):
    return [(r["nmatches"], r["match_of_train"]) for r in _kf_search(self, problems, partial_ok, mode)]


ORBmatcher.KfSearch = _kf_search
# SearchByProjection(pKF, Scw, vpPoints, vpMatched, th): [(nmatches, match_of_train)]
ORBmatcher.SearchByProjectionSim3 = lambda self, problems, partial_ok=False: _kf_search_tuples(self, problems, 0, partial_ok)
# Fuse(pKF, Scw, vpPoints, th, vpReplacePoint): [(best_idx, best_dist)]
ORBmatcher.FuseSim3 = lambda self, problems, partial_ok=False: [(r["best_idx"], r["best_dist"]) for r in _kf_search(self, problems, partial_ok, 1)]
# SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist): [(nmatches, match_of_train)]
ORBmatcher.SearchByProjectionKeyFrame = lambda self, problems, partial_ok=False: _kf_search_tuples(self, problems, 2, partial_ok)
ORBmatcher.SearchBySim3 = _search_by_sim3
