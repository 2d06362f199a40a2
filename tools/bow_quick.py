"""Developer tool: the bag-of-words calls at the workload's own shape.  A seeded full k = 10, L = 6 tree (1 111 110 nodes, 35.6 MB
of node descriptors); ps_bow_transform on 512 frames x 2000 features (8 distinct descriptor sets, each used 64 times) and on one
frame; ps_search_by_bow on 512 problems of 2000 x 2000 features over about 100 nodes (8 distinct seeded pairs with descriptor
families), both overloads, and on one problem.  Prints the kernel time of a call (ps_matcher_last_kernel_ms: bow_walk +
bow_vector, or bow_search + bow_commit) and the wall time of the C call, median of 5 after 2 warm-up calls, and the rate of the
descent over its 1920 bytes per feature (6 levels x 10 children x 32 B).  --json PATH writes the figures as JSON."""
import ctypes, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pointslot_amd import bow, keyframes, matcher as M
from pointslot_amd._lib import lib, check

K, L, NFEAT, NFRAMES, NODES, DISTINCT = 10, 6, 2000, 512, 100, 8
out = {"k": K, "L": L, "features": NFEAT, "batch": NFRAMES}
rng = np.random.default_rng(0xB0)
# the tree in breadth-first record order: level d holds K^d nodes, the children of a node are consecutive records
counts = [K ** d for d in range(1, L + 1)]
first = np.concatenate([[1], 1 + np.cumsum(counts)])          # node id of the first node of level d + 1
parent = np.concatenate([np.zeros(K, np.int64)] + [np.repeat(np.arange(first[d - 1], first[d]), K) for d in range(1, L)]).astype(np.int32)
nn = len(parent)
desc = rng.integers(0, 256, (nn, 32), dtype=np.uint8)
is_leaf = np.zeros(nn, np.uint8); is_leaf[-counts[-1]:] = 1
weight = np.where(is_leaf != 0, rng.uniform(0.1, 8.0, nn), 0.0).astype(np.float32)
t0 = time.perf_counter()
voc = bow.Vocabulary.from_arrays(K, L, bow.TF_IDF, parent, desc, weight, is_leaf)
out["vocabulary_create_ms"] = (time.perf_counter() - t0) * 1e3
print("vocabulary: %s, created in %.0f ms" % (voc.info(), out["vocabulary_create_ms"]), flush=True)
m = M.ORBmatcher(0.7, True)


def timed(call):
    ker, wall = [], []
    for it in range(7):
        t0 = time.perf_counter()
        check(call())
        wall.append((time.perf_counter() - t0) * 1e3)
        ker.append(m.last_kernel_ms())
    return float(np.median(ker[2:])), float(np.median(wall[2:]))


sets = [rng.integers(0, 256, (NFEAT, 32), dtype=np.uint8) for _ in range(DISTINCT)]
for count in (1, NFRAMES):
    arr = (bow._BowProblem * count)()
    keep = []
    for i in range(count):
        o = dict(word=np.zeros(NFEAT, np.int32), node=np.zeros(NFEAT, np.int32), bow_id=np.zeros(NFEAT, np.int32), bow_val=np.zeros(NFEAT, np.float64))
        p = arr[i]
        p.n, p.desc, p.levelsup = NFEAT, sets[i % DISTINCT].ctypes.data, 4
        for name, v in o.items():
            setattr(p, name, v.ctypes.data)
        keep.append(o)
    ker, wall = timed(lambda: lib.ps_bow_transform(m._h, voc._h, arr, count))
    rate = count * NFEAT * L * K * 32 / (ker * 1e-3) / 1e12
    out["transform_%d" % count] = dict(kernel_ms=ker, call_ms=wall, descent_tb_per_s=rate, words=int(arr[0].bow_n))
    print("transform %3d frames per call: kernels %.3f ms, call %.2f ms, %.2f TB/s over 1920 B per feature (%d words in frame 0)"
          % (count, ker, wall, rate, arr[0].bow_n), flush=True)

pairs = [keyframes.bow_pair(0xB0B0 + i, na=NFEAT, nb=NFEAT, n_nodes=NODES, families=(300, 6, 8)) for i in range(DISTINCT)]
for mode in (0, 1):
    for count in (1, NFRAMES):
        arr = (M._BowSearchProblem * count)()
        keep = []
        for i in range(count):
            a, b = pairs[i % DISTINCT]
            p = arr[i]
            p.mode = mode
            M._fill_bow_side(p.a, a, keep, True)
            M._fill_bow_side(p.b, b, keep, True)
            match = np.zeros(NFEAT, np.int32)
            p.nn_ratio, p.check_orientation, p.match = 0.7, 1, match.ctypes.data
            keep.append(match)
        ker, wall = timed(lambda: lib.ps_search_by_bow(m._h, arr, count))
        out["search_mode%d_%d" % (mode, count)] = dict(kernel_ms=ker, call_ms=wall, kernel_us_per_pair=ker * 1e3 / count, matches=int(arr[0].nmatches))
        print("search mode %d, %3d problems per call: kernels %.3f ms (%.2f us per pair), call %.2f ms (%d matches in problem 0)"
              % (mode, count, ker, ker * 1e3 / count, wall, arr[0].nmatches), flush=True)
if "--json" in sys.argv[1:]:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
