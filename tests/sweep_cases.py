"""The scenes of the randomised sweeps over the mapping and place-recognition calls (tools/stress_{tri,bow,kfdb,kfsearch}.py) and of
tests/test_sweep_cases_cpu.py: calls(family, seed, budget) is a deterministic list of calls drawn from shape lists that step over
every kernel's chunk sizes (a wave, a 256-thread workgroup, the 64-entry resolve chunk, 4096 and 8192-bit bitmaps, the 64-word
prefetch of the database's wave sum), so every consumer sees the same bytes.  Pure numpy on pointslot_amd.keyframes,
bow.synthetic_vocabulary, kfsearch_cases._main / _sim3 and kfdb_cases._vector; no GPU code.  references(family, seed, budget) are the
second opinions' answers, call by call, computed once per process.  Test infrastructure."""
import functools

import numpy as np

import bow_cases
import bow_second_opinion as bow_so
import kfdb_cases
import kfsearch_cases as kc
import kfsearch_second_opinion as ks_so
import tri_second_opinion as tri_so
from pointslot_amd import bow, keyframes, matcher, synth

F32 = np.float32
I32 = np.int32
# the seed and the budget tests/test_random_sweeps_gpu.py runs each tool with; tests/test_sweep_cases_cpu.py checks these very runs
COMMITTED = {"tri": (20250601, 60), "bow": (20250602, 20), "kfdb": (20250603, 60), "kfsearch": (20250604, 45),
             "stereo": (20250605, 26),                                    # (the stereo matcher's scenes: tests/stereo_cases.py)
             "match": (20250606, 39)}                                     # (the tracking thread's matchers: tests/match_cases.py)

TRI_N1 = (1, 63, 64, 65, 255, 256, 257, 513, 1100)
TRI_N2 = (1, 63, 64, 65, 130, 257, 600)
TRI_K = (1, 2, 3, 5)
TRI_NODES = (1, 2, 5, 12, 40)
BOW_TREES = ((2, 6), (3, 5), (10, 4), (16, 2), (17, 3), (20, 2))          # (k, L); (10, 4) has 10^4 words
BOW_BIG = (10, 4)
BOW_N = (0, 1, 2, 3, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1025, 2000)
BOW_SIDES = (1, 63, 64, 65, 129, 700, 2000)
BOW_NODES = (1, 2, 12, 40)
KFDB_STORED = (0, 1, 63, 64, 65, 127, 128, 129, 700, 2000)
KFDB_QUERY = (1, 64, 65, 500, 2000)
KS_NF = (1, 63, 64, 65, 257, 2000, 4097)
KS_NQ = (1, 3, 4, 5, 63, 64, 65, 300, 2000)
KS_CAP = 32                                                               # candidates a point keeps in the everyday store


class _Draw:
    """choices from pointslot_amd.synth's generator: the same on every machine"""

    def __init__(self, seed):
        self.rng = synth.Rng(seed)

    def u(self):
        return float(self.rng.uniform(1)[0])

    def chance(self, p):
        return self.u() < p

    def int(self, lo, hi):
        """uniform in [lo, hi]"""
        return int(self.rng.integers(1, lo, hi + 1)[0])

    def pick(self, seq):
        return seq[int(self.rng.integers(1, 0, len(seq))[0])]

    def seed(self):
        return self.int(1, (1 << 30) - 1)


# ---- CreateNewMapPoints --------------------------------------------------------------------------------------------------------
def _tri_problem(d, forced=None):
    s = dict(n1=d.pick(TRI_N1), k=d.pick(TRI_K), n_nodes=d.pick(TRI_NODES), only_stereo=int(d.chance(0.25)), check_orientation=int(d.chance(0.6)),
             chain=int(d.chance(0.7)), p_occupied=d.pick((0.0, 0.05, 0.25)), noise=d.pick((0.3, 0.5, 2.0)), flip_bits=d.pick((0, 10, 16)),
             raw_shift=d.pick((0.0, 0.0, 0.75)), families=d.pick((None, None, (40, 6, 8))), seed=d.seed())
    s["k"] = (forced or {}).get("k", s["k"])
    s["n2"] = [d.pick(TRI_N2) for _ in range(s["k"])]
    s["step"] = [0.0] + [d.pick((0.3, 0.7, 1.0, 1.0, 2.0)) * (i + 1) if d.chance(0.5) else 1.0 * (i + 1) for i in range(s["k"])]
    if forced:
        s.update(forced)
    kfs = keyframes.keyframe_set(s["seed"], n_kf=1 + s["k"], sizes=[s["n1"]] + list(s["n2"]), n_nodes=s["n_nodes"], step=s["step"], noise=s["noise"],
                                 flip_bits=s["flip_bits"], p_occupied=s["p_occupied"], raw_shift=s["raw_shift"], descriptor_families=s["families"])
    pr = keyframes.problem_of(kfs, s["only_stereo"], s["check_orientation"], 1, s["chain"])
    pr["settings"] = s
    return pr


def _tri_calls(seed, budget):
    d = _Draw(seed)
    out, n = [], 0
    while n < budget:
        size = min(d.int(2, 5) if d.chance(0.4) else 1, budget - n)
        probs = []
        for _ in range(size):
            forced = None
            if n == 2:          # the one problem with 32 neighbours
                forced = dict(k=32, n1=60, n2=[60] * 32, n_nodes=4, step=[0.7 * i for i in range(33)])
            elif n == 5:        # node lists longer than a wave, chained, so that created points block the later neighbours
                forced = dict(n1=513, k=3, n2=[257, 600, 130], n_nodes=2, chain=1, p_occupied=0.05, only_stereo=0, step=[0.0, 1.0, 2.0, 3.0])
            elif n == 9:        # a neighbour below the baseline between two that are not
                forced = dict(k=3, step=[0.0, 1.0, 0.3, 2.0])
            probs.append(_tri_problem(d, forced))
            n += 1
        # keyframe 1 through a frame handle now and then (the tool publishes it); unequal n1: the grid is sized by the largest
        out.append(dict(problems=probs, from_frame=[d.chance(0.2) and len(p["kf1"]["node"]) > 0 for p in probs]))
    return out


def tri_bad_pairs(ref):
    """the input condition of the x3d comparison (tests/test_tri_cpu.py::test_seeded_cases_are_well_posed): the pairs whose verdict
    does not survive +-1 float32 ulp, or whose A has sigma1 / sigma3 > 1e5"""
    return [p for p in ref["pairs"] if not p["stable"] or (p["kind"] == "svd" and not p["ratio"] <= 1e5)]


# ---- bag of words --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bow_vocabulary(seed, k, L):
    """the sweep's tree for (k, L): the four weightings, pruning, stopped words and tied siblings spread over the trees"""
    i = BOW_TREES.index((k, L))
    small = (k, L) != BOW_BIG
    return bow.synthetic_vocabulary(seed * 16 + i, k=k, L=L, p_prune=0.2 if small and L > 2 else 0.0, p_stop=0.1 if small else 0.02,
                                    tie_siblings=0.3 if small else 0.05, weighting=i % 4)


@functools.lru_cache(maxsize=None)
def bow_second_opinion_vocabulary(seed, k, L):
    v = bow_vocabulary(seed, k, L)
    return bow_so.Vocab(v["k"], v["L"], v["weighting"], v["parent"], v["desc"], v["weight"], v["is_leaf"])


def _bow_features(v, n, seed, bases):
    """bases == 0: bow_cases.features_for (many distinct words); otherwise n copies of `bases` descriptors in a shuffled order -
    after the sort, runs of n / bases equal words that cross the chunks of bow_vector"""
    if bases == 0 or n == 0:
        return bow_cases.features_for(v, n, seed)
    rng = synth.Rng(seed)
    pool = bow_cases.features_for(v, bases, seed + 1)
    return np.ascontiguousarray(pool[rng.integers(n, 0, bases)])


def _bow_transform_call(d, seed, forced=None, tree=None):
    k, L = d.pick(BOW_TREES) if tree is None else tree
    sizes = [d.pick(BOW_N) for _ in range(d.pick((1, 2, 3, 5)))]
    mixes = [d.pick((0, 0, 1, 2, 3, 7)) for _ in sizes]
    if forced:
        (k, L), sizes, mixes = forced
    v = bow_vocabulary(seed, k, L)
    frames = [_bow_features(v, n, d.seed(), m) for n, m in zip(sizes, mixes)]
    return dict(kind="transform", tree=(k, L), frames=frames, mixes=mixes, levelsup=[d.pick((0, 1, L - 1, L, L + 3)) for _ in sizes])


def _bow_search_call(d, forced=None):
    probs = []
    for j in range(d.pick((1, 2, 3, 5))):
        na, nb = d.pick(BOW_SIDES), d.pick(BOW_SIDES)
        if forced and j == 0:
            na, nb = forced
        if na == nb == 2000 and not forced:
            nb = 700            # one 2000 x 2000 pair is forced; more would not fit a few seconds of second opinion
        big = max(min(na, nb), 8)
        a, b = keyframes.bow_pair(d.seed(), na=na, nb=nb, n_nodes=d.pick(BOW_NODES), families=(max(big // 8, 1), 6, 8), flip_bits=d.pick((4, 8)),
                                  p_point=d.pick((0.0, 0.3, 0.8, 1.0)))
        probs.append(dict(a=a, b=b, mode=d.pick((0, 1)), nn_ratio=d.pick((0.6, 0.75, 0.9)), check_orientation=int(d.chance(0.5))))
    return dict(kind="search", problems=probs)


def _bow_calls(seed, budget):
    """transform and search calls in turn (the tool makes them on one matcher handle)"""
    d = _Draw(seed)
    out = []
    for i in range(budget):
        if i == 0:          # > 1000 distinct words, and runs of hundreds of equal words, both past n = 1025
            out.append(_bow_transform_call(d, seed, (BOW_BIG, [2000, 1025, 17, 2000, 513], [0, 3, 0, 2, 1])))
        elif i == 1:
            out.append(_bow_search_call(d, (2000, 2000)))
        elif i % 2 == 0:        # every tree (and with them every weighting) once, then any
            out.append(_bow_transform_call(d, seed, tree=BOW_TREES[(BOW_TREES.index(BOW_BIG) + i // 2) % len(BOW_TREES)] if i // 2 < len(BOW_TREES) else None))
        else:
            out.append(_bow_search_call(d))
    return out


# ---- the keyframe database -------------------------------------------------------------------------------------------------------
def _kfdb_queries(d, rng, W, stored, qid, modes, place=None):
    """place: the first query asks about the place after it, the others about it - a relocalisation query draws part of its words
    from the next place's pool, so keyframes there that the first query scored are listed, unscored, with a score left behind"""
    out = []
    for k, mode in enumerate(modes):
        p = d.int(0, len(W["pools"]) - 1) if place is None else (place + (k == 0)) % len(W["pools"])
        n = d.pick(KFDB_QUERY + (150, 260)) if not d.chance(0.1) else 2000
        # (a pool holds 360 words: a longer query draws its other words from the whole vocabulary, or it would come out short)
        bw = kfdb_cases._vector(rng, W["pools"], p, n, foreign=(p + 1) % len(W["pools"]) if mode == 0 and n <= 300 else None)
        connected, min_score = [], 0.0
        if mode == 1 and stored:
            ranked = sorted(stored, key=lambda x: -kfdb_cases._words_in_common(bw, W["kfs"][x]))
            connected = ranked[:2] + W["neigh"].get(ranked[0], [])[:2] + [kfdb_cases.OUTSIDERS[k % len(kfdb_cases.OUTSIDERS)]]
            sc = [kfdb_cases.so.score(list(zip(*bw)), list(zip(*W["kfs"][c]))) for c in connected if c in stored]
            min_score = float(F32(0.5 * min(sc))) if sc else 0.0
        out.append(dict(qid=qid + k, bow=bw, mode=mode, connected=connected, min_score=min_score))
    return out


def _kfdb_lengths_case(seed, n_kf):
    """random adds, erases, re-adds, a clear, queries in calls of 1 .. 8 and scores over stored vectors of every listed length"""
    d, rng = _Draw(seed), synth.Rng(seed + 1)
    pools = [np.sort(kfdb_cases._sample(rng, np.arange(kfdb_cases.NWORDS), kfdb_cases.POOL)) for _ in range(4)]
    ids = [1000 + 7 * i for i in range(n_kf)]
    # most vectors have 230 .. 300 words, so that a query scores several of them; the short ones of the list sit among them, and the
    # two long ones come with the last adds (a stored vector that holds every word of every query is the only one scored)
    lengths = [d.int(230, 300) for _ in range(n_kf)]
    third = n_kf // 3
    for j, n in zip(np.argsort(rng.uniform(2 * third), kind="stable"), KFDB_STORED[:8]):
        lengths[int(j)] = n
    lengths[2 * third + 1], lengths[n_kf - 2] = KFDB_STORED[8], KFDB_STORED[9]
    kfs = {x: kfdb_cases._vector(rng, pools, i % 4, lengths[i]) for i, x in enumerate(ids)}
    neigh = {}
    for i, x in enumerate(ids):
        same = [y for j, y in enumerate(ids) if j % 4 == i % 4 and y != x]
        after = [y for j, y in enumerate(ids) if j % 4 == (i + 1) % 4]
        got = []
        for _ in range(d.int(0, 10)):
            u = d.u()
            y = d.pick(same) if u < 0.6 else d.pick(after) if u < 0.9 else d.pick(ids + kfdb_cases.OUTSIDERS)
            if y != x and y not in got:
                got.append(y)
        neigh[x] = got
    W = dict(pools=pools, kfs=kfs, neigh=neigh)
    ops, stored, qid = [], [], [100]

    def ask(nq, place=None):
        modes = [0 if place is not None or d.chance(0.6) else 1 for _ in range(nq)]
        ops.append(("query", _kfdb_queries(d, rng, W, list(stored), qid[0], modes, place)))
        qid[0] += nq

    def add(xs):
        ops.append(("add", list(xs))); stored.extend(xs)
    add(ids[:third]); ask(d.int(1, 8))
    add(ids[third:2 * third]); ask(3, place=d.int(0, 3)); ask(d.int(2, 8))      # three relocalisation queries score the same slots
    gone = [stored[j] for j in sorted(set(d.int(0, len(stored) - 1) for _ in range(7)))] + [stored[-1]]
    gone = list(dict.fromkeys(gone))
    ops.append(("erase", gone + [123456]))
    stored[:] = [x for x in stored if x not in gone]
    ask(d.int(1, 8))
    add(gone[:3]); add(ids[2 * third:]); ask(5, place=d.int(0, 3)); ask(d.int(1, 8))
    q = _kfdb_queries(d, rng, W, list(stored), 0, [0, 0])
    ops.append(("score", q[0]["bow"], list(stored))); ops.append(("score", q[1]["bow"], list(stored)[::-3]))
    ops.append(("clear",)); stored[:] = []
    add(ids[1::5]); ask(d.int(1, 8))
    return dict(name="lengths", nwords=kfdb_cases.NWORDS, capacity=n_kf + 3, max_words=2000, kfs=kfs, neigh=neigh, ops=ops)


def _kfdb_many_case(seed, n_kf=2102):
    """about 2100 vectors of one to three words asked with 4 and with 6 queries: queries x slots lands in [8192, 16384), where a wave
    of kfdb_count serves 2 and 3 slots; 2102 slots are no multiple of 4"""
    d, rng = _Draw(seed), synth.Rng(seed + 1)
    nwords = 48
    kfs = {}
    for i in range(n_kf):
        w = np.sort(kfdb_cases._sample(rng, np.arange(nwords), 1 + i % 3)).astype(I32)
        v = rng.uniform(len(w), 0.05, 1.0)
        kfs[50 + i] = (w, v / v.sum())
    ids = sorted(kfs)
    neigh = {x: [d.pick(ids) for _ in range(i % 4)] for i, x in enumerate(ids[:400])}

    def q(qid, mode):
        w = np.sort(kfdb_cases._sample(rng, np.arange(nwords), d.int(2, 5))).astype(I32)
        v = rng.uniform(len(w), 0.05, 1.0)
        return dict(qid=qid, bow=(w, v / v.sum()), mode=mode, connected=[d.pick(ids) for _ in range(3)] if mode else [], min_score=0.0)
    ops = [("add", ids[:1000]), ("add", ids[1000:]), ("query", [q(1, 0), q(2, 1), q(3, 0), q(4, 0)]),
           ("query", [q(5, 1), q(6, 0), q(7, 0), q(8, 1), q(9, 0), q(10, 0)])]
    return dict(name="many", nwords=nwords, capacity=n_kf + 2, max_words=4, kfs=kfs, neigh=neigh, ops=ops)


def _kfdb_calls(seed, budget):
    return [_kfdb_lengths_case(seed, budget), _kfdb_many_case(seed + 7)]


def kfdb_high(case):
    """per query op of a case: (queries, high) - high is one past the highest slot in use; a stored keyframe takes the lowest free
    slot (include/pointslot_hip.h)"""
    slot, free, cap, out = {}, [], 0, []
    for op in case["ops"]:
        if op[0] == "add":
            for x in op[1]:
                if free:
                    free.sort(); slot[x] = free.pop(0)
                else:
                    slot[x] = cap; cap += 1
        elif op[0] == "erase":
            for x in op[1]:
                if x in slot:
                    free.append(slot.pop(x))
        elif op[0] == "clear":
            slot, free, cap = {}, [], 0
        elif op[0] == "query":
            out.append((len(op[1]), max(slot.values()) + 1 if slot else 0))
    return out


# ---- the keyframe searches -------------------------------------------------------------------------------------------------------
_TRAIN_KEYS = ("x", "y", "octave", "angle", "occupied", "desc")


def _reorder_train(pr, order):
    """the searched side's features in another order (feature i moves to where order says i is: new[j] = old[order[j]])"""
    kc._reordered(pr, order)
    if "dense" in pr:
        inv = np.argsort(order)
        pr["dense"]["features"] = inv[pr["dense"]["features"]]


def _shuffle_train(pr, rng, high=None):
    """a random feature order; high: this many of the first (projected-from, likely matched) features go to the highest indices"""
    n = len(pr["train"]["x"])
    order = np.argsort(rng.uniform(n), kind="stable")
    if high and n > high:
        first = np.arange(high)
        order = np.concatenate([order[~np.isin(order, first)], first])
    _reorder_train(pr, order)


def _dense(mode, seed, th, th_dist, nplain, first):
    """kfsearch_cases._wide inside a plain scene: 300 features within half a search radius of one pixel, every one within th_dist of the
    points projected there - more takeable candidates than the 32 the everyday store keeps, so the problem takes the wide re-run"""
    pr = kc._main(mode, seed, nf=nplain, nq=nplain, th=th, first=first, th_dist=th_dist, check_orientation=int(seed % 2))
    rng = np.random.RandomState(seed + 5)
    t, q = pr["train"], pr["query"]
    sc = kc._Scene(rng, mode, (pr["R"], pr["t"], pr["ow"]))
    base = kc._new_desc(rng)
    r = th * 1.2 ** 4
    cu, cv = rng.uniform(200, 1000), rng.uniform(150, 300)
    for k in range(300):
        sc.feature(cu + rng.uniform(-r / 2, r / 2), cv + rng.uniform(-r / 2, r / 2), 4, kc._flip(rng, base, int(rng.randint(2, 30))),
                   angle=rng.uniform(0, 360), occupied=int(k % 50 == 0))
    for k in range(12):
        sc.point(kc._cam_of_pixel(cu + rng.uniform(-1, 1), cv + rng.uniform(-1, 1), 10.0), kc._flip(rng, base, int(rng.randint(0, 6))), 4, angle=rng.uniform(0, 360))
    extra = sc.problem(th)
    n0, m0 = len(t["x"]), len(q["valid"])
    for k in _TRAIN_KEYS:
        t[k] = np.concatenate([t[k], extra["train"][k]])
    for k in q:
        q[k] = np.concatenate([q[k], extra["query"][k]])
    t["cell_off"], t["cell_idx"] = matcher.build_grid(t["x"], t["y"], *kc.GRID)
    pr["dense"] = dict(features=np.arange(n0, n0 + 300), points=np.arange(m0, m0 + 12), level=4)
    return pr


def _ks_kf_call(d, forced=None):
    probs = []
    for j in range(d.pick((1, 2, 3, 4))):
        mode = d.pick((0, 1, 2))
        nf, nq = d.pick(KS_NF), d.pick(KS_NQ)
        dense = mode != 1 and d.chance(0.3)
        if forced and j < len(forced):
            mode, nf, nq, dense = forced[j]
        th, th_dist = d.pick((3.0, 4.0, 10.0)), d.pick((50, 64, 100))
        seed, first = d.seed(), d.int(0, 28)
        if dense:
            pr = _dense(mode, seed, th, th_dist, d.pick((63, 65, 257)), first)
        else:
            pr = kc._main(mode, seed, nf=nf, nq=nq, th=th, spread=d.chance(0.3), first=first, th_dist=th_dist, check_orientation=int(d.chance(0.7)))
        _shuffle_train(pr, synth.Rng(seed), high=8 if nf == 4097 and not dense else None)
        probs.append(pr)
    return dict(kind="kf", problems=probs, from_frame=[d.chance(0.2) and len(p["train"]["x"]) > 0 for p in probs])


_SIDE_KEYS = ("x", "y", "octave", "angle", "desc", "has_point", "pos", "min_dist", "max_dist", "point_desc", "already")


def _shuffle_side(kf, rng, last):
    """a keyframe of a Sim3 problem with its features (and the points in their slots) in a random order; the features `last` go to
    the highest indices"""
    n = len(kf["x"])
    order = np.argsort(rng.uniform(n), kind="stable")
    order = np.concatenate([order[~np.isin(order, last)], np.asarray(last, np.int64)])
    for k in _SIDE_KEYS:
        kf[k] = np.ascontiguousarray(kf[k][order])
    kf["cell_off"], kf["cell_idx"] = matcher.build_grid(kf["x"], kf["y"], *kc.GRID)


def _ks_sim3_call(d, forced=None):
    probs = []
    for j in range(d.pick((1, 2, 3))):
        n = d.pick((1, 63, 64, 65, 257, 2000))
        if forced and j == 0:
            n = forced
        seed = d.seed()
        pr = kc._sim3(seed, d.pick((1.0, 0.93, 1.07)), n=n, tie=d.chance(0.3) and n >= 200)
        del pr["expect_tie"]                                      # (indices before the shuffle)
        rng = synth.Rng(seed)
        m12 = ks_so.search_by_sim3(pr)["match12"] if n > 4096 else np.zeros(0, I32)      # eight agreed pairs end above index 4088
        top = np.flatnonzero(m12 >= 0)[:8]
        _shuffle_side(pr["kf1"], rng, top); _shuffle_side(pr["kf2"], rng, m12[top])
        probs.append(pr)
    return dict(kind="sim3", problems=probs)


def _kfsearch_calls(seed, budget):
    """budget: problems, in calls of 1 .. 4; a Sim3 call after every three keyframe-search calls"""
    d = _Draw(seed)
    out, n, i = [], 0, 0
    while n < budget:
        if i == 0:          # a dense problem beside plain ones of every ordered mode; matches above index 4096
            c = _ks_kf_call(d, [(0, 4097, 2000, False), (2, 0, 0, True), (1, 257, 65, False), (0, 0, 0, True)])
        elif i == 1:
            c = _ks_kf_call(d, [(2, 4097, 2000, False), (0, 65, 64, False)])
        elif i == 3:
            c = _ks_sim3_call(d, 4097)
        elif i % 4 == 3:
            c = _ks_sim3_call(d)
        else:
            c = _ks_kf_call(d)
        out.append(c)
        n += len(c["problems"]); i += 1
    return out


def level_violations(ref):
    """the input condition of the keyframe searches (tests/test_kfsearch_cpu.py::test_input_condition_of_the_gpu_comparison): how many
    predicted levels change when log(ratio) / logScale moves by +- 4 ulp, or have ratio within 4 float ulp of a power of 1.2"""
    ok = np.isfinite(ref["logv"])
    lv, ratio = ref["logv"][ok], ref["ratio"][ok]
    clamp = lambda v: np.clip(np.ceil(v), 0, 7)
    step = 4 * np.spacing(np.abs(lv))
    bad = clamp(lv - step) != clamp(lv + step)
    powers = np.array([1.2 ** k for k in range(-60, 61)])
    gap = np.abs(ratio.astype(np.float64)[:, None] - powers[None, :]).min(axis=1) if len(ratio) else np.zeros(0)
    return int((bad | ~(gap > 4 * np.spacing(ratio).astype(np.float64))).sum()), int(ok.sum())


def takeable_bound(pr, ref, dense):
    """dense: a LOWER bound on the candidates the points of the dense window keep (features of the cluster - all inside every such
    point's window by construction - that are free, at the point's level or the one below, and within th_dist; 0 unless the second
    opinion searched the point at all).  Otherwise an UPPER bound for every point of the problem: free features within th_dist
    anywhere in the image."""
    t, q = pr["train"], pr["query"]
    th_dist = int(pr.get("th_dist", 100)) if pr["mode"] == 2 else 50          # ORBdist; TH_LOW for the Sim3 overload
    free = t["occupied"] == 0
    if dense:
        f, lv = pr["dense"]["features"], pr["dense"]["level"]
        free = free[f] & (t["octave"][f] >= lv - 1) & (t["octave"][f] <= lv)
        feats, points = t["desc"][f], [i for i in pr["dense"]["points"] if ref["gate"][i] in ("match", "nomatch")]
    else:
        feats, points = t["desc"], range(len(q["valid"]))
    pop = np.array([bin(i).count("1") for i in range(256)], np.int32)
    counts = [int(((pop[feats ^ q["desc"][i][None, :]].sum(axis=1) <= th_dist) & free).sum()) for i in points]
    return (min(counts) if dense else max(counts)) if counts else 0


# ---- the public face -------------------------------------------------------------------------------------------------------------
_FAMILIES = {"tri": _tri_calls, "bow": _bow_calls, "kfdb": _kfdb_calls, "kfsearch": _kfsearch_calls}


@functools.lru_cache(maxsize=None)
def calls(family, seed, budget):
    """the sweep of one family: a list of calls (tri, kfsearch: dict(problems, from_frame) / dict(kind="sim3", problems); bow:
    dict(kind="transform", tree, frames, levelsup) / dict(kind="search", problems); kfdb: kfdb_cases scripts).  The arrays are shared:
    do not write into them."""
    return _FAMILIES[family](int(seed), int(budget))


def reference_of(family, seed, call):
    """the second opinion's answers to one call, problem by problem"""
    if family == "tri":
        return [tri_so.create_new_map_points(p) for p in call["problems"]]
    if family == "bow":
        if call["kind"] == "transform":
            voc = bow_second_opinion_vocabulary(seed, *call["tree"])
            return [voc.transform(f, lv) for f, lv in zip(call["frames"], call["levelsup"])]
        return [bow_so.search_by_bow(p["a"], p["b"], p["mode"], p["nn_ratio"], p["check_orientation"]) for p in call["problems"]]
    if family == "kfdb":
        return kfdb_cases.play_second_opinion(call)
    if call["kind"] == "sim3":
        return [ks_so.search_by_sim3(p) for p in call["problems"]]
    return [ks_so.run(p) for p in call["problems"]]


@functools.lru_cache(maxsize=None)
def references(family, seed, budget):
    return [reference_of(family, int(seed), c) for c in calls(family, seed, budget)]
