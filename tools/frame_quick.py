"""What a per-call SearchByProjection costs with the train side uploaded per call and with it in a frame handle (developer tool).

One problem: SearchByProjection(cur, last, th) with n = 2000 train keypoints and 1500 queries (synth.projection_scene, seed
0x51070020).  Per variant the median over 200 calls after 20 warm-up calls of the wall time around the C call and of
ps_matcher_last_kernel_ms; for the frames variant also the time of one publish (host arrays / from the extractor) by HIP events.

  tools/frame_quick.py --variant host|frames        one process, one JSON line
  tools/frame_quick.py --all [--parent-lib build_exp/libps_parent.so] [--kitti build/stereo_kitti] [--out profiles/frame_quick.json]
      five fresh processes per variant, interleaved: (a) the parent commit's library through PS_LIB_PATH, host arrays; (b) this
      library, host arrays; (c) this library, frame handle.  Median and range over the processes.  --kitti: examples/stereo_kitti
      on a generated 154-frame sequence with PS_ODO_DEVICE_FRAMES off and on (three processes each).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS, WARMUP, PROCESSES = 200, 20, 5


def one_process(variant):
    import numpy as np
    from pointslot_amd import synth
    from pointslot_amd._lib import lib, check
    from pointslot_amd.matcher import ORBmatcher, build_grid
    sc = synth.projection_scene(0x51070020, n=2000, m=1500)
    tr = dict(sc["train"])
    tr["cell_off"], tr["cell_idx"] = build_grid(tr["x"], tr["y"], *tr["grid"])
    pr = {"train": tr, "scale_factors": sc["scale_factors"], "mode": "frame", "query": sc["frame_query"], "tcw": sc["tcw"], "tlw": sc["tlw"],
          "K6": sc["K6"], "bounds": sc["bounds"], "th": sc["th"]}
    m = ORBmatcher(0.9, True)
    out = {"variant": variant, "lib": os.environ.get("PS_LIB_PATH", "")}
    F = None
    if variant == "frames":
        from pointslot_amd.frame import DeviceFrame
        F = DeviceFrame(2048)
        F.publish(tr, tr["u_right"], tr["desc"], tr["grid"])
        pr = dict(pr, train={"frame": F, "occupied": tr["occupied"], "in_bbox": tr["in_bbox"]})
    arr, frames, keep, outs = m._prepare_projection([pr])
    if frames is None:
        call = lambda: lib.ps_search_by_projection(m._h, arr, 1)
    else:
        call = lambda: lib.ps_search_by_projection_frames(m._h, arr, frames, 1)
    wall, kern = [], []
    for k in range(WARMUP + CALLS):
        t0 = time.perf_counter()
        rc = call()
        t1 = time.perf_counter()
        check(rc)
        if k >= WARMUP:
            wall.append((t1 - t0) * 1e3); kern.append(m.last_kernel_ms())
    out.update(nmatches=int(arr[0].nmatches), wall_ms=statistics.median(wall), kernel_ms=statistics.median(kern))
    if F is not None:
        ms = []
        for k in range(WARMUP + CALLS):
            F.publish(tr, tr["u_right"], tr["desc"], tr["grid"])
            ms.append(F.last_publish_ms())
        out["publish_host_ms"] = statistics.median(ms[WARMUP:])
        t0 = time.perf_counter()
        for k in range(CALLS):
            F.publish(tr, tr["u_right"], tr["desc"], tr["grid"])
        F.last_publish_ms()
        out["publish_host_wall_ms"] = (time.perf_counter() - t0) * 1e3 / CALLS      # back to back, the upload of one behind the kernel of the other
        from pointslot_amd.extractor import ORBextractor
        L, R = synth.stereo_pair()
        ex = ORBextractor(2000, 1.2, 8, 20, 5, max_batch=2)
        ex.extract_batch([L, R])
        ex.stereo_match_batch(1, np.float32(384.38148 / 721.5377), np.float32(384.38148))
        n = len(ex.stereo_fetch_frames(1)[0][0])
        grid = (0.0, 0.0, 64.0 / L.shape[1], 48.0 / L.shape[0])
        E = DeviceFrame(ex.capacity)
        ms = []
        for k in range(WARMUP + CALLS):
            E.publish_from(ex, 0, 0, n, grid)
            ms.append(E.last_publish_ms())
        out.update(publish_orb_ms=statistics.median(ms[WARMUP:]), publish_orb_n=n)
        ex.close(); E.close(); F.close()
    m.close()
    print(json.dumps(out))


def _spread(rows, key):
    v = [r[key] for r in rows if key in r]
    return None if not v else {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def run_all(parent_lib, kitti, out_path):
    variants = [("b_this_host_arrays", "host", None), ("c_this_frame_handle", "frames", None)]
    if parent_lib:
        variants.insert(0, ("a_parent_host_arrays", "host", os.path.abspath(parent_lib)))
    rows = {name: [] for name, _, _ in variants}
    for rep in range(PROCESSES):                      # interleaved: a drift of the machine lands on every variant alike
        for name, variant, libpath in variants:
            env = dict(os.environ)
            env.pop("PS_LIB_PATH", None)
            if libpath:
                env["PS_LIB_PATH"] = libpath
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", variant], capture_output=True, text=True, env=env, timeout=600)
            if r.returncode != 0:
                raise SystemExit("%s failed:\n%s%s" % (name, r.stdout[-2000:], r.stderr[-2000:]))
            rows[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(name, rows[name][-1], flush=True)
    result = {"problem": "SearchByProjection(cur, last, th): 2000 train keypoints, 1500 queries, seed 0x51070020", "calls": CALLS, "warmup": WARMUP,
              "processes": PROCESSES, "variants": {}}
    for name in rows:
        result["variants"][name] = {k: _spread(rows[name], k) for k in ("wall_ms", "kernel_ms", "publish_host_ms", "publish_host_wall_ms", "publish_orb_ms")
                                    if _spread(rows[name], k) is not None}
        result["variants"][name]["nmatches"] = rows[name][0]["nmatches"]
    if kitti:
        from pointslot_amd import sequence
        seq = sequence.generate(n_frames=154, seed=4)
        with tempfile.TemporaryDirectory() as tmp:
            d = os.path.join(tmp, "0000")
            sequence.write(d, seq, pgm=True)
            runs = {"off": [], "on": []}
            traj = {}
            for rep in range(3):
                for switch in ("off", "on"):
                    env = dict(os.environ)
                    env.pop("PS_ODO_DEVICE_FRAMES", None)
                    if switch == "on":
                        env["PS_ODO_DEVICE_FRAMES"] = "1"
                    r = subprocess.run([os.path.abspath(kitti), d], capture_output=True, text=True, env=env, timeout=900)
                    if r.returncode != 0:
                        raise SystemExit("stereo_kitti (%s) failed:\n%s%s" % (switch, r.stdout[-2000:], r.stderr[-2000:]))
                    lines = r.stdout.splitlines()
                    split = json.loads([l for l in lines if l.startswith("split_json:")][-1][len("split_json:"):])
                    split["median_tracking_ms"] = float([l for l in lines if l.startswith("median tracking time:")][-1].split()[3])
                    runs[switch].append(split)
                    traj[switch] = open(os.path.join(d, "CameraTrajectory.txt"), "rb").read()
                    print("stereo_kitti", switch, split, flush=True)
            keys = ("median_tracking_ms", "wall_ms", "stereo_call_ms", "search_call_ms", "search_kernels_ms", "host_marshalling_ms")
            result["stereo_kitti_154_frames"] = {s: {k: _spread(runs[s], k) for k in keys} for s in runs}
            result["stereo_kitti_154_frames"]["same_trajectory"] = traj["off"] == traj["on"]
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["host", "frames"])
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--kitti")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.all:
        run_all(a.parent_lib, a.kitti, a.out)
    else:
        one_process(a.variant or "host")
