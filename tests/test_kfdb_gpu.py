"""The keyframe database on the device (pointslot_amd/kfdb.py over ps_kfdb_*) against the second opinion
(tests/kfdb_second_opinion.py) on the cases of tests/kfdb_cases.py.  Everything is equal, not close: the sharing lists and their
order, the word counts, the scores (float bits), min_common_words, the candidate lists of both modes and ps_kfdb_score (double
bits)."""
import functools

import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_second_opinion as so
import parity_checks

pytestmark = pytest.mark.gpu

F32 = np.float32


_play = parity_checks.play_kfdb_device


@functools.lru_cache(maxsize=None)
def _device(name):
    from pointslot_amd import kfdb
    case = kc.CASES[name]()
    db = kfdb.KeyFrameDatabase(case["capacity"], case["max_words"])
    return _play(db, case), db


_same = parity_checks.check_kfdb_query


@pytest.mark.parametrize("name", ["hand", "a", "b", "batch", "batch_split"])
def test_query_equals_the_second_opinion(name):
    got, _ = _device(name)
    want = kc.second_opinion(name)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _same(g, w, (name, w["query"]["qid"]))


def test_vectors_at_the_word_limit():
    """a stored vector and a query of 8191 words: the sharing lists, the scores of both modes and ps_kfdb_score"""
    got, _ = _device("limit")
    want = kc.second_opinion("limit")
    assert len(got) == len(want) == 3 and len(want[0]["share_id"]) == 5 and (want[0]["share_score"] > 0).sum() >= 2
    for g, w in zip(got[:2], want[:2]):
        _same(g, w, ("limit", w["query"]["qid"]))
    assert (want[2]["scores"] > 0).all()
    parity_checks.check_kfdb_score(got[2]["scores"], want[2]["scores"], "limit")


def test_hand_case_as_written():
    got, _ = _device("hand")
    for g, w in zip(got, kc.HAND_EXPECTED):
        _same(g, dict(w, share_score=np.array(w["share_score"], F32)), w)


def test_batch_equals_one_query_per_call():
    one, _ = _device("batch")
    split, _ = _device("batch_split")
    assert len(one) == len(split) == 7
    for a, b in zip(one, split):
        _same(a, b, "batch against split")


@pytest.mark.parametrize("name", ["hand", "a", "b"])
def test_score_equals_the_sequential_double_sum(name):
    _, db = _device(name)
    case = kc.CASES[name]()
    stored = kc.stored_after(name)
    assert len(db) == len(stored)
    for r in kc.second_opinion(name)[-3:]:
        q = r["query"]
        got = db.score(q["bow"], stored)
        want = np.array([so.score(list(zip(*q["bow"])), list(zip(*case["kfs"][i]))) for i in stored])
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), q["qid"]
    if name == "hand":
        got = db.score(kc._bow(kc.HAND_Q1), kc.HAND_SCORE_IDS)
        assert got.tobytes() == np.array(kc.HAND_SCORES).tobytes()


def test_score_of_an_unknown_id_is_nan_and_an_error():
    from pointslot_amd._lib import PointslotError, PS_ERR_INVALID
    _, db = _device("hand")
    q = kc._bow(kc.HAND_Q1)
    with pytest.raises(PointslotError) as e:
        db.score(q, [10, 777])
    assert e.value.code == PS_ERR_INVALID
    got = db.score(q, [10, 777, 13], unknown_ok=True)
    assert got[0] == 0.75 and np.isnan(got[1]) and got[2] == 0.5


def test_reference_named_calls_on_the_hand_case():
    from pointslot_amd import KeyFrameDatabase
    case = kc.hand_case()
    db = KeyFrameDatabase(case["capacity"], case["max_words"])
    db.add(sorted(case["kfs"]), [case["kfs"][i] for i in sorted(case["kfs"])])
    for op, want in zip(case["ops"][1:], kc.HAND_EXPECTED):
        q = op[1][0]
        if q["mode"] == 1:
            got = db.detect_loop_candidates(q["bow"], q["connected"], q["min_score"], case["neigh"])
        else:
            got = db.detect_relocalization_candidates(q["bow"], case["neigh"])
        assert got == want["candidates"]


def test_empty_database_empty_query_and_clear():
    from pointslot_amd import kfdb
    case = kc.hand_case()
    ids = sorted(case["kfs"])
    db = kfdb.KeyFrameDatabase(8, 8)
    empty = (np.zeros(0, np.int32), np.zeros(0, np.float64))
    q1 = kc._bow(kc.HAND_Q1)
    for mode in (0, 1):
        r = db.query([dict(bow=q1, mode=mode), dict(bow=empty, mode=mode)])
        assert [len(x["share_id"]) for x in r] == [0, 0] and all(x["min_common_words"] == 0 and not x["failed"] for x in r)
    assert len(db) == 0
    db.add(ids, [case["kfs"][i] for i in ids])
    assert len(db) == 6
    r = db.query([dict(bow=empty, mode=0), dict(bow=q1, mode=0)])
    assert len(r[0]["share_id"]) == 0 and r[0]["min_common_words"] == 0 and kfdb.select(0, 0.0, r[0], case["neigh"]) == []
    assert [int(x) for x in r[1]["share_id"]] == kc.HAND_EXPECTED[0]["share_id"]
    db.clear()
    assert len(db) == 0
    assert len(db.query([dict(bow=q1, mode=0)])[0]["share_id"]) == 0
    # after clear the database is as new: the same adds give the same lists, and reloc_score starts at 0 again
    db.add(ids, [case["kfs"][i] for i in ids])
    r = db.query([dict(bow=q1, mode=0)])[0]
    assert [int(x) for x in r["share_id"]] == kc.HAND_EXPECTED[0]["share_id"]
    assert r["share_score"].tobytes() == np.array(kc.HAND_EXPECTED[0]["share_score"], F32).tobytes()
    db.erase([10, 4242])                                # an unknown id is ignored
    assert len(db) == 5
    r = db.query([dict(bow=q1, mode=0)])[0]
    assert [int(x) for x in r["share_id"]] == [13, 11, 14, 12]


def test_errors_and_entries_that_fail_alone():
    from pointslot_amd import kfdb
    from pointslot_amd._lib import PointslotError, PS_ERR_INVALID, PS_ERR_CAPACITY
    case = kc.hand_case()
    db = kfdb.KeyFrameDatabase(4, 5)
    assert db.add([10, 11], [case["kfs"][10], case["kfs"][11]]) == [True, True]
    with pytest.raises(PointslotError) as e:            # a stored id: nothing of the batch is stored
        db.add([12, 10], [case["kfs"][12], case["kfs"][10]])
    assert e.value.code == PS_ERR_INVALID and len(db) == 2
    with pytest.raises(PointslotError) as e:            # ids not ascending
        db.add([12], [(np.array([3, 2], np.int32), np.array([.5, .5]))])
    assert e.value.code == PS_ERR_INVALID and len(db) == 2
    long = (np.arange(6, dtype=np.int32), np.full(6, 1 / 6))
    with pytest.raises(PointslotError) as e:
        db.add([20], [long])
    assert e.value.code == PS_ERR_CAPACITY and len(db) == 2
    # a vector longer than max_words fails alone; then the database is full and the last entry fails alone
    got = db.add([12, 20, 13, 14], [case["kfs"][12], long, case["kfs"][13], case["kfs"][14]], partial_ok=True)
    assert got == [True, False, True, False] and len(db) == 4
    r = db.query([dict(bow=kc._bow(kc.HAND_Q1), mode=0)])[0]
    assert [int(x) for x in r["share_id"]] == [10, 13, 11, 12] and list(r["share_words"]) == [4, 4, 2, 1]
    db.erase([11])
    assert db.add([14], [case["kfs"][14]]) == [True]    # the freed slot is taken again
    r = db.query([dict(bow=kc._bow(kc.HAND_Q1), mode=0)])[0]
    assert [int(x) for x in r["share_id"]] == [10, 13, 14, 12]
    with pytest.raises(PointslotError) as e:
        kfdb.KeyFrameDatabase(kfdb.MAX_CAPACITY + 1, 8)
    assert e.value.code == PS_ERR_INVALID
    with pytest.raises(PointslotError) as e:
        kfdb.KeyFrameDatabase(8, kfdb.MAX_WORDS + 1)
    assert e.value.code == PS_ERR_INVALID
    # a query beyond the limit fails alone
    big = (np.arange(kfdb.MAX_WORDS + 1, dtype=np.int32), np.full(kfdb.MAX_WORDS + 1, 1e-4))
    r = db.query([dict(bow=big, mode=0), dict(bow=kc._bow(kc.HAND_Q1), mode=1, excluded=[10])], partial_ok=True)
    assert r[0]["failed"] and not r[1]["failed"] and [int(x) for x in r[1]["share_id"]] == [13, 14, 12]


def test_full_capacity_database():
    """4096 keyframes, the documented limit: the list kernel sorts all of them in one workgroup"""
    from pointslot_amd import kfdb
    n = kfdb.MAX_CAPACITY
    db = kfdb.KeyFrameDatabase(n, 4)
    # keyframe i holds word i % 7 (and word 9 when i % 3 == 0); the query holds words 2, 5 and 9
    bows = [(np.array([i % 7, 9] if i % 3 == 0 else [i % 7], np.int32), np.array([.5, .5] if i % 3 == 0 else [1.0])) for i in range(n)]
    assert all(db.add(np.arange(n) + 50, bows))
    q = (np.array([2, 5, 9], np.int32), np.array([.25, .25, .5]))
    r = db.query([dict(bow=q, mode=0)])[0]
    want = [i for i in range(n) if i % 7 == 2] + [i for i in range(n) if i % 7 == 5] + [i for i in range(n) if i % 3 == 0 and i % 7 not in (2, 5)]
    assert [int(x) - 50 for x in r["share_id"]] == want
    assert r["min_common_words"] == 1 and list(r["share_words"]) == [2 if i % 3 == 0 and i % 7 in (2, 5) else 1 for i in want]
    scored = r["share_words"] > 1
    assert np.all(r["share_score"][scored] == F32(0.75)) and np.all(r["share_score"][~scored] == 0)
    # a batch over the nearly full database: kfdb_count gives a wave several slots, and the last workgroup runs past the end.
    # Every value is a multiple of 1/4, so the score is the exact sum of min(v, w) over the common words.
    db.erase(np.arange(n - 6, n) + 50)
    live = list(range(n - 6))
    reloc = {i: F32(0.75) if i % 3 == 0 and i % 7 in (2, 5) else F32(0) for i in live}

    def expect(bow, mode, excluded=()):
        qd = dict(zip(bow[0].tolist(), bow[1].tolist()))
        rows = sorted((min(w for w in bows[i][0].tolist() if w in qd), i, sum(w in qd for w in bows[i][0].tolist()))
                      for i in live if not (mode == 1 and i + 50 in excluded) and any(w in qd for w in bows[i][0].tolist()))
        mincw = int(F32(max(w for _, _, w in rows)) * F32(0.8))
        fresh = {i: F32(sum(min(qd[x], v) for x, v in zip(bows[i][0].tolist(), bows[i][1].tolist()) if x in qd)) for _, i, w in rows if w > mincw}
        if mode == 0:
            reloc.update(fresh)
        score = [reloc[i] if mode == 0 else fresh.get(i, F32(0)) for _, i, _ in rows]
        return [i + 50 for _, i, _ in rows], [w for _, _, w in rows], np.array(score, F32), mincw
    q2 = (np.array([0, 9], np.int32), np.array([.5, .5]))
    batch = [dict(bow=q, mode=1, excluded=[50 + 2, 50 + 51]), dict(bow=q2, mode=0), dict(bow=q, mode=1), dict(bow=q2, mode=1, excluded=[50]), dict(bow=q, mode=0)]
    for x, r in zip(batch, db.query(batch)):
        ids, words, score, mincw = expect(x["bow"], x["mode"], x.get("excluded", ()))
        assert [int(v) for v in r["share_id"]] == ids and list(r["share_words"]) == words
        assert r["share_score"].tobytes() == score.tobytes() and r["min_common_words"] == mincw


def test_vectors_straight_from_the_transform():
    """BowVectors as ps_bow_transform writes them, added and queried untouched"""
    import bow_cases as bc
    from pointslot_amd import bow, kfdb
    name = "full_k10_L3"
    voc = bow.Vocabulary.from_arrays(**bc.vocabulary(name))
    feat = bc.transform_features(name)
    frames = [feat[0:120], feat[60:200], feat[150:300], feat[::2], feat[30:170]]
    res = voc.transform(frames, levelsup=1)
    bows = [(r["bow_id"], r["bow_val"]) for r in res]
    assert all(len(b[0]) > 20 for b in bows)
    db = kfdb.KeyFrameDatabase(8, 300)
    db.add([1, 2, 3, 4], bows[:4])
    ref = so.KeyFrameDatabase(voc.size())
    kfs = [so.KeyFrame(i + 1, *bows[i]) for i in range(4)]
    for k in kfs:
        ref.add(k)
    kfs[0].neigh, kfs[1].neigh = [kfs[1], kfs[3]], [kfs[0]]
    neigh = {1: [2, 4], 2: [1]}
    query = so.KeyFrame(-7, *bows[4])
    cand, tr = ref.DetectRelocalizationCandidates(query)
    r = db.query([dict(bow=bows[4], mode=0)])[0]
    assert len(tr["share"]) >= 3
    assert [int(x) for x in r["share_id"]] == tr["share"] and list(r["share_words"]) == tr["words"]
    assert r["share_score"].tobytes() == np.array(tr["score"], F32).tobytes() and r["min_common_words"] == tr["min_common_words"]
    assert kfdb.select(0, 0.0, r, neigh) == [c.mnId for c in cand]
    want = np.array([so.score(query.mBowVec, k.mBowVec) for k in kfs])
    assert db.score(bows[4], [1, 2, 3, 4]).tobytes() == want.tobytes()
