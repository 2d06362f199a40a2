"""Cases for the keyframe database tests.  A case is a script: kfs = {id: BowVector}, neigh = {id: ordered ids of
GetBestCovisibilityKeyFrames(10)} (ids that are never stored included), and ops - ("add", ids), ("erase", ids), ("clear",),
("score", bow, ids) for ps_kfdb_score or ("query", [queries]) for one call serving several queries.  A query is a dict: qid, bow, mode (0 relocalisation, 1 loop),
connected (the ids of GetConnectedKeyFrames()) and min_score.  second_opinion() plays a case through tests/kfdb_second_opinion.py
once and is shared by all tests.  The sizes are small: seconds on the GPU; the workload's 1500-word vectors are for
tools/kfdb_quick.py."""
import functools

import numpy as np

import kfdb_second_opinion as so
from pointslot_amd import synth

F32 = np.float32
I32 = np.int32


def _bow(d):
    ids = sorted(d)
    return np.array(ids, I32), np.array([d[w] for w in ids], np.float64)


# ---- the hand case: a 12-word vocabulary, 6 keyframes ---------------------------------------------------------------------------
# Every value is a multiple of 1/8, so every sum below is exact; for positive values the term fabs(v - w) - fabs(v) - fabs(w) is
# -2 min(v, w) and the score is the sum of min(v, w) over the common words.
#   A 10 {1: 1/4, 2: 1/4, 3: 1/4, 4: 1/4}            neighbours D, B, F
#   B 11 {2: 1/2, 3: 1/4, 5: 1/4}                     neighbours A, E
#   C 12 {0: 1/2, 6: 1/2}
#   D 13 {1: 1/8, 2: 1/8, 3: 1/4, 4: 1/4, 7: 1/4}     neighbours A, 99 (never stored)
#   E 14 {4: 1/2, 8: 1/2}
#   F 15 {9: 1}
# Q1 = {1: 1/4, 2: 1/4, 3: 1/8, 4: 1/8, 6: 1/4}, relocalisation.  Word 1 lists A, D; word 2 adds B; word 4 adds E; word 6 adds C:
#   the list is A D B E C with 4 4 2 1 1 words; max 4, min = int(3.2f) = 3; A and D are scored: 1/4 + 1/4 + 1/8 + 1/8 = 3/4 and
#   4 x 1/8 = 1/2; the others keep reloc_score 0.  A: + D 1/2 + B 0 (shares a word, unscored), F not listed: acc 5/4, best A.
#   D: + A 3/4 which beats 1/2: acc 5/4, best A.  Retain > 15/16: A, then A again - a duplicate.  Candidates [10].
# Q2 = {2: 1/2, 5: 1/4, 7: 1/4}, relocalisation.  Word 2 lists A, B, D: the list is A B D with 1 2 2 words; max 2, min = int(1.6f)
#   = 1; B: 1/2 + 1/4 = 3/4, D: 1/8 + 1/4 = 3/8; A is not scored and still holds Q1's 3/4.  B: + A 3/4 (stale), E not listed: acc
#   3/2, best B (3/4 > 3/4 is false).  D: + A 3/4: acc 9/8, best A.  Retain > 9/8: B stays, (9/8, A) is rejected.  Candidates [11].
# Q3 = Q1's vector, loop, connected {A, 99}, minScore 0.3.  A is never listed: D B E C with 4 2 1 1; max 4, min 3; D scored 1/2 >=
#   0.3; its neighbour A is not in the list, 99 neither: acc 1/2 > 0.3.  Candidates [13].  Scores reported: 1/2 0 0 0.
# Q4 = Q1's vector, loop, connected {A, D}, minScore 0.3.  B E C with 2 1 1; max 2, min 1; B scored 1/4 + 1/8 = 3/8; neighbour A
#   excluded, E has 1 word, not > 1: acc 3/8.  Candidates [11].  Without the exclusion the maximum would have been 4.
# Q5 = as Q4 with minScore 0.4: 3/8 < 0.4, nothing is retained.  Candidates [].
# ps_kfdb_score(Q1; A, D, B, F) = 3/4, 1/2, 3/8, -0.0 (no common word: the sum stays 0 and -0/2 is -0).
HAND_KFS = {10: {1: .25, 2: .25, 3: .25, 4: .25}, 11: {2: .5, 3: .25, 5: .25}, 12: {0: .5, 6: .5}, 13: {1: .125, 2: .125, 3: .25, 4: .25, 7: .25},
            14: {4: .5, 8: .5}, 15: {9: 1.0}}
HAND_NEIGH = {10: [13, 11, 15], 11: [10, 14], 13: [10, 99]}
HAND_Q1 = {1: .25, 2: .25, 3: .125, 4: .125, 6: .25}
HAND_Q2 = {2: .5, 5: .25, 7: .25}
HAND_EXPECTED = [
    dict(share_id=[10, 13, 11, 14, 12], share_words=[4, 4, 2, 1, 1], share_score=[.75, .5, 0., 0., 0.], min_common_words=3, candidates=[10]),
    dict(share_id=[10, 11, 13], share_words=[1, 2, 2], share_score=[.75, .75, .375], min_common_words=1, candidates=[11]),
    dict(share_id=[13, 11, 14, 12], share_words=[4, 2, 1, 1], share_score=[.5, 0., 0., 0.], min_common_words=3, candidates=[13]),
    dict(share_id=[11, 14, 12], share_words=[2, 1, 1], share_score=[.375, 0., 0.], min_common_words=1, candidates=[11]),
    dict(share_id=[11, 14, 12], share_words=[2, 1, 1], share_score=[.375, 0., 0.], min_common_words=1, candidates=[]),
]
HAND_SCORE_IDS = [10, 13, 11, 15]
HAND_SCORES = [.75, .5, .375, -0.0]


def hand_case():
    q1, q2 = _bow(HAND_Q1), _bow(HAND_Q2)
    queries = [dict(qid=1, bow=q1, mode=0, connected=[], min_score=0.0), dict(qid=2, bow=q2, mode=0, connected=[], min_score=0.0),
               dict(qid=3, bow=q1, mode=1, connected=[10, 99], min_score=0.3), dict(qid=4, bow=q1, mode=1, connected=[10, 13], min_score=0.3),
               dict(qid=5, bow=q1, mode=1, connected=[10, 13], min_score=0.4)]
    return dict(nwords=12, capacity=8, max_words=8, kfs={k: _bow(v) for k, v in HAND_KFS.items()}, neigh=HAND_NEIGH,
                ops=[("add", sorted(HAND_KFS))] + [("query", [q]) for q in queries])


# ---- the seeded cases ------------------------------------------------------------------------------------------------------------
NWORDS, NPLACES, POOL = 2000, 5, 360
OUTSIDERS = [9000 + i for i in range(6)]              # keyframes of the map that are never stored
SPECIAL_LENGTHS = {3: 0, 11: 1, 17: 63, 22: 64, 29: 65, 31: 300, 44: 299, 58: 128}


def _sample(rng, pool, n):
    pool = np.asarray(pool)
    return pool[np.argsort(rng.uniform(len(pool)), kind="stable")[:n]]


def _vector(rng, pools, place, n, foreign=None):
    """n words: most from the place's pool, the rest from anywhere (or from the pool of place `foreign`); values L1-normalised as
    ps_bow_transform leaves them"""
    if n == 0:
        return np.zeros(0, I32), np.zeros(0, np.float64)
    inside = min(int(round(0.85 * n)), n)
    words = set(int(w) for w in _sample(rng, pools[place], inside))
    other = np.arange(NWORDS) if foreign is None else pools[foreign]
    for w in _sample(rng, other, len(other)):
        if len(words) >= n:
            break
        words.add(int(w))
    ids = np.array(sorted(words), I32)
    val = rng.uniform(len(ids), 0.05, 1.0)
    return ids, val / val.sum()


def _kf_id(i):
    return 2 ** 40 + 5 if i == 20 else 1000 + 7 * i     # ids are the caller's: sparse, one beyond 32 bits


@functools.lru_cache(maxsize=None)
def _world():
    rng = synth.Rng(4100)
    pools = [np.sort(_sample(rng, np.arange(NWORDS), POOL)) for _ in range(NPLACES)]
    n_kf = 70 + 3                                      # 70 for case A, 3 more that case B adds
    lengths = rng.integers(n_kf, 230, 300)
    kfs, place = {}, {}
    for i in range(n_kf):
        n = SPECIAL_LENGTHS.get(i, int(lengths[i]))
        kfs[_kf_id(i)] = _vector(rng, pools, i % NPLACES, n)
        place[_kf_id(i)] = i % NPLACES
    ids = list(kfs)
    neigh = {}
    for k in ids:
        n = min(10, int(11 * (1.0 - float(rng.uniform(1)[0]) ** 4)))       # 0 .. 10, mostly many
        same = [x for x in ids if place[x] == place[k] and x != k]
        out = []
        for u, pick in zip(rng.uniform(n), rng.uniform(n)):
            src = same if u < 0.75 else ids if u < 0.9 else OUTSIDERS
            x = src[int(pick * len(src))]
            if x != k and x not in out:
                out.append(x)
        neigh[k] = out
    return dict(pools=pools, kfs=kfs, place=place, neigh=neigh, ids=ids)


def _words_in_common(a, b):
    return len(np.intersect1d(a[0], b[0]))


# one seed per query, tuned until every query of the seeded cases ends with at least two candidates (tests/test_kfdb_cpu.py)
SEEDS = {"a": [510, 511, 512, 513, 514, 515], "b": [1020, 521, 522, 523, 524, 525], "batch": [530, 531, 532, 533, 534, 835, 536]}


def _queries(seeds, stored, first_qid, modes, foreign_step=1):
    """one query per entry of modes, walking through the places.  A relocalisation query draws part of its words from another place's
    pool: keyframes there share words without being scored.  A loop query is connected to the stored keyframes that share the
    most words with it and to their first neighbours, so an excluded keyframe would have had the most words."""
    W = _world()
    out = []
    for k, mode in enumerate(modes):
        rng = synth.Rng(seeds[k])
        p = k % NPLACES
        bow = _vector(rng, W["pools"], p, int(rng.integers(1, 150, 260)[0]), foreign=(p + foreign_step) % NPLACES if mode == 0 else None)
        connected = []
        if mode == 1:
            ranked = sorted(stored, key=lambda x: -_words_in_common(bow, W["kfs"][x]))
            connected = ranked[:2] + W["neigh"][ranked[0]][:2] + [OUTSIDERS[k % len(OUTSIDERS)]]
        out.append(dict(qid=first_qid + k, bow=bow, mode=mode, connected=connected, min_score=0.0))
    for q in out:
        if q["mode"] == 1:
            # LoopClosing::DetectLoop: the least score against a connected keyframe; halved so that it cuts the list somewhere
            sc = [so.score(list(zip(*q["bow"])), list(zip(*W["kfs"][c]))) for c in q["connected"] if c in W["kfs"] and c in stored]
            q["min_score"] = float(F32(0.5 * min(sc)))
    return out


@functools.lru_cache(maxsize=None)
def case_a():
    W = _world()
    stored = W["ids"][:70]
    return dict(nwords=NWORDS, capacity=80, max_words=320, kfs=W["kfs"], neigh=W["neigh"],
                ops=[("add", stored[:40]), ("add", stored[40:])] + [("query", [q]) for q in _queries(SEEDS["a"], stored, 100, [0, 1, 0, 1, 0, 1])])


ERASED = [0, 69, 35, 5, 12, 22, 41, 50, 63]            # positions in add order: the first, the last, a middle one, six more
READDED = [35, 0, 50, 12]


@functools.lru_cache(maxsize=None)
def case_b():
    """case A's database after erasing 9 keyframes, adding 4 of them again and adding 3 new ones"""
    W = _world()
    a = case_a()
    ids = W["ids"]
    stored = [x for i, x in enumerate(ids[:70]) if i not in ERASED] + [ids[i] for i in READDED] + ids[70:]
    return dict(a, ops=a["ops"] + [("erase", [ids[i] for i in ERASED] + [123456]), ("add", [ids[i] for i in READDED]), ("add", ids[70:])]
                + [("query", [q]) for q in _queries(SEEDS["b"], stored, 200, [1, 0, 1, 0, 1, 0])])


BATCH_MODES = [0, 0, 1, 0, 0, 1, 0]


@functools.lru_cache(maxsize=None)
def case_batch(split=False):
    """five relocalisation and two loop queries in one call - or, split, the same seven one per call"""
    W = _world()
    stored = W["ids"][:70]
    qs = _queries(SEEDS["batch"], stored, 300, BATCH_MODES, foreign_step=4)
    return dict(nwords=NWORDS, capacity=70, max_words=300, kfs=W["kfs"], neigh=W["neigh"],
                ops=[("add", stored)] + ([("query", [q]) for q in qs] if split else [("query", qs)]))


@functools.lru_cache(maxsize=None)
def case_limit():
    """one stored vector and one query of 8191 words (MAX_WORDS), beside shorter ones: 128 chunks of the wave sum's 64-word prefetch,
    the whole 32 KB query in LDS, 13-step binary searches; query in both modes and ps_kfdb_score"""
    rng = synth.Rng(4200)
    nwords = 12000

    def vec(n):
        ids = np.sort(_sample(rng, np.arange(nwords), n)).astype(I32)
        val = rng.uniform(n, 0.05, 1.0)
        return ids, val / val.sum()
    kfs = {1: vec(8191), 2: vec(300), 3: vec(8000), 4: vec(65), 5: vec(6000)}
    q = vec(8191)
    queries = [dict(qid=1, bow=q, mode=0, connected=[], min_score=0.0), dict(qid=2, bow=q, mode=1, connected=[3], min_score=0.0)]
    return dict(nwords=nwords, capacity=5, max_words=8191, kfs=kfs, neigh={1: [3, 5], 3: [1], 5: [2, 1]},
                ops=[("add", [1, 2, 3, 4, 5]), ("query", queries), ("score", q, [1, 2, 3, 4, 5])])


CASES = {"limit": case_limit, "hand": hand_case, "a": case_a, "b": case_b, "batch": case_batch, "batch_split": functools.partial(case_batch, True)}


@functools.lru_cache(maxsize=None)
def second_opinion(name):
    """one result per query, in the order the case asks them: share_id, share_words, share_score, min_common_words, candidates,
    the query itself and the second opinion's trace"""
    return play_second_opinion(CASES[name]())


def play_second_opinion(case):
    """The ops interpreter: a case script played through tests/kfdb_second_opinion.py.  One result per query, in order; an op
    ("score", bow, ids) - ps_kfdb_score against stored keyframes - gives dict(scores=float64 array) in its place in that order."""
    db = so.KeyFrameDatabase(case["nwords"])
    obj = {}                                           # every keyframe of the map; an erased one that is added again is a new object

    def get(i):
        if i not in obj:
            obj[i] = so.KeyFrame(i)
        return obj[i]
    stored = {}
    out = []
    for op in case["ops"]:
        if op[0] == "add":
            for i in op[1]:
                obj[i] = stored[i] = so.KeyFrame(i, *case["kfs"][i])
                db.add(obj[i])
        elif op[0] == "erase":
            for i in op[1]:
                if i in stored:
                    db.erase(stored.pop(i))
        elif op[0] == "clear":
            db.clear()
            stored.clear()
        elif op[0] == "score":
            out.append(dict(scores=np.array([so.score(list(zip(*op[1])), list(zip(*case["kfs"][i]))) for i in op[2]], np.float64)))
        else:
            for k in list(obj.values()):
                k.neigh = [get(x) for x in case["neigh"].get(k.mnId, [])]
            for q in op[1]:
                kf = so.KeyFrame(-1000 - q["qid"], *q["bow"])
                kf.connected = set(get(x) for x in q["connected"])
                if q["mode"] == 1:
                    cand, tr = db.DetectLoopCandidates(kf, q["min_score"])
                else:
                    cand, tr = db.DetectRelocalizationCandidates(kf)
                out.append(dict(share_id=np.array(tr["share"], np.int64), share_words=np.array(tr["words"], I32),
                                share_score=np.array(tr["score"], F32), min_common_words=tr["min_common_words"],
                                candidates=[c.mnId for c in cand], query=q, trace=tr))
    return out


def stored_after(name):
    """the ids the database holds when the case has been played, in add order"""
    live = []
    for op in CASES[name]()["ops"]:
        if op[0] == "add":
            live += list(op[1])
        elif op[0] == "erase":
            live = [x for x in live if x not in op[1]]
        elif op[0] == "clear":
            live = []
    return live
