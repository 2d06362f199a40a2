"""Developer tool: the keyframe database at the workload's shape.  Databases of 256, 1024 and 4096 keyframes with about 1500
words each out of 10^5, drawn as places of 16 keyframes (85 % of a keyframe's words from its place's pool of 2000, as in
tests/kfdb_cases.py).  Per size: the time to add the whole database in one call; the kernel time (ps_matcher_last_kernel_ms:
kfdb_count + kfdb_score + kfdb_list) and the wall time of one ps_kfdb_query call with 1 and with 16 relocalisation queries -
median of 20 calls after 3 warm-up calls, with the least and the greatest; and the time of the same queries through a
single-threaded host inverted file structured as the reference's (tools/kfdb_host_invfile.cpp, built here with g++ -O2).
The two sides are compared on what they computed: the length of the sharing list and the number of scored keyframes.
--json PATH writes the figures as JSON."""
import ctypes, json, os, subprocess, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
from pointslot_amd import kfdb
from pointslot_amd._lib import lib, check, _KfdbQueryProblem

NWORDS, LEN, PER_PLACE, POOL, WARM, REPS = 100000, 1500, 16, 2000, 3, 20
SIZES = (256, 1024, 4096)
if "--sizes" in sys.argv[1:]:                        # e.g. --sizes 4096: one size only, for a kernel trace
    SIZES = tuple(int(x) for x in sys.argv[sys.argv.index("--sizes") + 1].split(","))
rng = np.random.default_rng(0xDB)


def vector(pool):
    ids = np.unique(np.concatenate([rng.choice(pool, int(0.85 * LEN), replace=False), rng.integers(0, NWORDS, LEN - int(0.85 * LEN))])).astype(np.int32)
    val = rng.uniform(0.05, 1.0, len(ids))
    return ids, val / val.sum()


tmp = tempfile.mkdtemp()
so_path = os.path.join(tmp, "libkfdb_host_invfile.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so_path, os.path.join(HERE, "kfdb_host_invfile.cpp")])
ivf = ctypes.CDLL(so_path)
ivf.ivf_create.restype = ctypes.c_void_p
ivf.ivf_create.argtypes = [ctypes.c_int]
ivf.ivf_destroy.argtypes = [ctypes.c_void_p]
ivf.ivf_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
ivf.ivf_query.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]


def stats(x):
    return dict(median=float(np.median(x)), least=float(np.min(x)), greatest=float(np.max(x)))


out = {"words": NWORDS, "words_per_keyframe": LEN, "keyframes_per_place": PER_PLACE, "warmup": WARM, "repeats": REPS, "sizes": {}}
for size in SIZES:
    pools = [rng.choice(NWORDS, POOL, replace=False) for _ in range(size // PER_PLACE)]
    bows = [vector(pools[i % len(pools)]) for i in range(size)]
    queries = [vector(pools[(7 * q) % len(pools)]) for q in range(16)]
    db = kfdb.KeyFrameDatabase(size, 2048)
    t0 = time.perf_counter()
    db.add(np.arange(size) + 1, bows)
    add_ms = (time.perf_counter() - t0) * 1e3
    host = ivf.ivf_create(NWORDS)
    for ids, val in bows:
        ivf.ivf_add(host, ids.ctypes.data, val.ctypes.data, len(ids))
    res = {"add_call_ms": add_ms, "mean_words": float(np.mean([len(b[0]) for b in bows]))}
    host_ms, host_counts = [], []
    for ids, val in queries:
        ms = np.zeros(WARM + REPS)
        nshare = ctypes.c_int(0)
        scored = ivf.ivf_query(host, ids.ctypes.data, val.ctypes.data, len(ids), WARM + REPS, ms.ctypes.data, ctypes.byref(nshare))
        host_ms.append(ms[WARM:])
        host_counts.append((nshare.value, scored))
    host_ms = np.array(host_ms)                      # [query][repetition]
    res["host_inverted_file_1_query_ms"] = stats(host_ms[0])
    res["host_inverted_file_16_queries_ms"] = stats(host_ms.sum(axis=0))
    for count in (1, 16):
        arr = (_KfdbQueryProblem * count)()
        keep = []
        for i in range(count):
            ids, val = queries[i]
            o = dict(share_id=np.zeros(size, np.int64), share_words=np.zeros(size, np.int32), share_score=np.zeros(size, np.float32))
            p = arr[i]
            p.n, p.bow_id, p.bow_val, p.mode, p.nexcluded, p.excluded = len(ids), ids.ctypes.data, val.ctypes.data, 0, 0, None
            for name, v in o.items():
                setattr(p, name, v.ctypes.data)
            keep.append(o)
        ker, wall = [], []
        for it in range(WARM + REPS):
            t0 = time.perf_counter()
            check(lib.ps_kfdb_query(db._h, db._m(), arr, count))
            wall.append((time.perf_counter() - t0) * 1e3)
            ker.append(db._matcher.last_kernel_ms())
        res["device_%d_kernel_ms" % count] = stats(ker[WARM:])
        res["device_%d_call_ms" % count] = stats(wall[WARM:])
        got = [(int(arr[i].nshare), int((keep[i]["share_words"][:arr[i].nshare] > arr[i].min_common_words).sum())) for i in range(count)]
        assert got == host_counts[:count], (got, host_counts[:count])
    res["sharing_and_scored_query_0"] = list(host_counts[0])
    ivf.ivf_destroy(host)
    db.close()
    out["sizes"][str(size)] = res
    print("%4d keyframes (%.0f words each): add %.1f ms | 1 query: kernels %.3f ms, call %.3f ms, host inverted file %.3f ms | 16 queries: kernels %.3f ms, "
          "call %.3f ms, host %.3f ms | query 0 shares words with %d, scores %d"
          % (size, res["mean_words"], add_ms, res["device_1_kernel_ms"]["median"], res["device_1_call_ms"]["median"], res["host_inverted_file_1_query_ms"]["median"],
             res["device_16_kernel_ms"]["median"], res["device_16_call_ms"]["median"], res["host_inverted_file_16_queries_ms"]["median"], *host_counts[0]), flush=True)
if "--json" in sys.argv[1:]:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
