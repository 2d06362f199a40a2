"""Developer tool: ps_create_new_map_points at the mapping thread's own shape - 2000 features per keyframe, 10 neighbours, about
100 vocabulary nodes - for 1 and for 512 keyframes per call, keyframe 1 from host arrays and from a DeviceFrame.  Prints the
kernel time of a call (ps_matcher_last_kernel_ms; with a handle it includes the staging copy out of the slab) and the wall time
of the C call, median of 5.  The 512 keyframes are 8 distinct seeded sets, each used 64 times.  --search-only: triangulate = 0."""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pointslot_amd import keyframes, matcher as M
from pointslot_amd._lib import lib, check
from pointslot_amd.frame import DeviceFrame

N, K, NODES, DISTINCT = 2000, 10, 100, 8
TRIANGULATE = 0 if "--search-only" in sys.argv[1:] else 1
GRID = (0.0, 0.0, np.float32(64) / np.float32(1241), np.float32(48) / np.float32(376))
m = M.ORBmatcher(0.6, False)
base = [keyframes.tri_problem(0x51070300 + i, k=K, n1=N, n2=N, n_nodes=NODES, step=0.8) for i in range(DISTINCT)]
frames = []
for pr in base:
    f = DeviceFrame(N)
    f.publish(pr["kf1"], pr["kf1"]["u_right"], pr["kf1"]["desc"], GRID)
    frames.append(f)


def prepared(count, handle):
    """the ps_tri_problem array of `count` keyframes, packed once: the timed loop is the C call alone"""
    arr = (M._TriProblem * count)()
    keep = []
    for i in range(count):
        pr, p = base[i % DISTINCT], arr[i]
        kf1 = pr["kf1"]
        if handle:
            kf1 = {k: v for k, v in kf1.items() if k not in ("x", "y", "octave", "angle", "u_right", "desc")}
        M._fill_tri_keyframe(p.kf1, kf1, keep, frames[i % DISTINCT] if handle else None)
        nb = (M._TriKeyframe * K)()
        for j, kf in enumerate(pr["kf2"]):
            M._fill_tri_keyframe(nb[j], kf, keep)
        f12 = np.ascontiguousarray(pr["f12"], np.float32).reshape(-1, 9)
        p.k, p.kf2, p.f12 = K, nb, f12.ctypes.data
        p.only_stereo, p.check_orientation, p.triangulate, p.chain, p.ratio_factor = 0, 0, TRIANGULATE, 1, float(pr["ratio_factor"])
        o = dict(match=np.zeros((K, N), np.int32), nmatches=np.zeros(K, np.int32), x3d=np.zeros((K, N, 3), np.float32),
                 status=np.zeros((K, N), np.uint8), nnew=np.zeros(1, np.int32))
        for name, v in o.items():
            setattr(p, name, v.ctypes.data)
        keep.append((nb, f12, o))
    handles = (ctypes.c_void_p * count)(*[frames[i % DISTINCT]._h.value for i in range(count)]) if handle else None
    return arr, handles, keep


for count in (1, 512):
    for handle in (False, True):
        arr, handles, keep = prepared(count, handle)
        ker, wall = [], []
        for it in range(7):
            t0 = time.perf_counter()
            check(lib.ps_create_new_map_points_frames(m._h, arr, handles, count) if handle else lib.ps_create_new_map_points(m._h, arr, count))
            wall.append((time.perf_counter() - t0) * 1e3)
            ker.append(m.last_kernel_ms())
        new = sum(int(k[2]["nnew"][0]) for k in keep if isinstance(k, tuple))
        print("%3d keyframes per call, keyframe 1 from %-12s: kernels %.3f ms, call %.2f ms (%d points created)"
              % (count, "a DeviceFrame" if handle else "host arrays", float(np.median(ker[2:])), float(np.median(wall[2:])), new), flush=True)
