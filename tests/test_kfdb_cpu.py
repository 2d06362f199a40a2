"""The keyframe database without a GPU: the second opinion (tests/kfdb_second_opinion.py) reproduces the hand case written out
in tests/kfdb_cases.py; the seeded cases exercise the branches they are meant to, judged on the second opinion alone; and
ps_kfdb_select - the host-only covisibility stage of the library - equals the second opinion's on every case."""
import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_second_opinion as so

F32 = np.float32


def test_second_opinion_reproduces_the_hand_case():
    got = kc.second_opinion("hand")
    assert len(got) == len(kc.HAND_EXPECTED)
    for g, want in zip(got, kc.HAND_EXPECTED):
        assert list(g["share_id"]) == want["share_id"]
        assert list(g["share_words"]) == want["share_words"]
        assert g["share_score"].tobytes() == np.array(want["share_score"], F32).tobytes()
        assert g["min_common_words"] == want["min_common_words"]
        assert g["candidates"] == want["candidates"]
    case = kc.hand_case()
    q1 = list(zip(*case["ops"][1][1][0]["bow"]))
    scores = [so.score(q1, list(zip(*case["kfs"][i]))) for i in kc.HAND_SCORE_IDS]
    assert np.array(scores).tobytes() == np.array(kc.HAND_SCORES).tobytes()
    # the hand case's own branches: a dropped duplicate (Q1), a stale read and a 0.75 rejection (Q2)
    assert got[0]["trace"]["duplicates"] == 1 and got[1]["trace"]["stale_reads"] == 2 and got[1]["trace"]["rejected"] == 1


def test_seeded_lengths_cover_the_chunk_edges():
    case = kc.case_a()
    stored = [i for op in case["ops"] if op[0] == "add" for i in op[1]]
    lengths = set(len(case["kfs"][i][0]) for i in stored)
    assert len(stored) == 70 and {0, 1, 63, 64, 65, 300} <= lengths
    for ids, val in case["kfs"].values():
        assert np.all(np.diff(ids) > 0) and (len(ids) == 0 or abs(val.sum() - 1) < 1e-12)
    b = kc.case_b()
    assert len(kc.stored_after("b")) == 70 - 9 + 4 + 3
    erase = [op for op in b["ops"] if op[0] == "erase"][0][1]
    first, last = kc.stored_after("a")[0], kc.stored_after("a")[-1]
    assert first in erase and last in erase


def _least_common(q, kf):
    return int(np.intersect1d(q[0], kf[0])[0])


@pytest.mark.parametrize("name", ["a", "b", "batch"])
def test_seeded_case_is_not_vacuous(name):
    res = kc.second_opinion(name)
    case = kc.CASES[name]()
    if name == "b":
        res = res[len(kc.second_opinion("a")):]           # the queries after the erases and adds
    tally = dict(best_is_neighbour=0, duplicates=0, rejected=0, stale_reads=0, ties_in_add_order=0, excluded_had_most=0)
    for r in res:
        assert len(r["share_id"]) >= 3 and len(r["candidates"]) >= 2, (r["query"]["qid"], len(r["share_id"]), r["candidates"])
        tr = r["trace"]
        for k in ("best_is_neighbour", "duplicates", "rejected", "stale_reads"):
            tally[k] += tr[k]
        least = [_least_common(r["query"]["bow"], case["kfs"][int(i)]) for i in r["share_id"]]
        assert least == sorted(least)
        tally["ties_in_add_order"] += sum(a == b for a, b in zip(least, least[1:]))
        if tr["mode"] == 1 and tr["excluded_words"] > max(r["share_words"]):
            tally["excluded_had_most"] += 1
    assert tally["best_is_neighbour"] >= 1 and tally["duplicates"] >= 1 and tally["rejected"] >= 1, tally
    assert tally["ties_in_add_order"] >= 1 and tally["excluded_had_most"] >= 1, tally
    if name == "batch":
        assert tally["stale_reads"] >= 1, tally
        modes = [r["query"]["mode"] for r in res]
        assert modes.count(0) == 5 and modes.count(1) == 2


def test_case_b_lists_show_the_new_serials():
    """a keyframe that was erased and added again stands behind every survivor with the same least common word"""
    W = kc._world()
    order = kc.stored_after("b")
    case = kc.case_b()
    readded = set(W["ids"][i] for i in kc.READDED)
    moved = 0
    for r in kc.second_opinion("b")[len(kc.second_opinion("a")):]:
        ids = [int(i) for i in r["share_id"]]
        least = [_least_common(r["query"]["bow"], case["kfs"][i]) for i in ids]
        for a, b, la, lb in zip(ids, ids[1:], least, least[1:]):
            if la == lb:
                assert order.index(a) < order.index(b)
                moved += a not in readded and b in readded and W["ids"].index(b) < W["ids"].index(a)
    assert moved >= 1


def test_batch_and_split_agree_in_the_second_opinion():
    one, split = kc.second_opinion("batch"), kc.second_opinion("batch_split")
    assert len(one) == len(split) == 7
    for a, b in zip(one, split):
        assert a["share_id"].tobytes() == b["share_id"].tobytes() and a["share_score"].tobytes() == b["share_score"].tobytes()
        assert a["candidates"] == b["candidates"]


@pytest.mark.parametrize("name", ["hand", "a", "b", "batch"])
def test_select_equals_the_second_opinions_covisibility_stage(name):
    from pointslot_amd import kfdb
    case = kc.CASES[name]()
    for r in kc.second_opinion(name):
        q = r["query"]
        got = kfdb.select(q["mode"], q["min_score"], r, case["neigh"])
        assert got == r["candidates"], q["qid"]


def test_select_rejects_bad_arguments():
    from pointslot_amd import kfdb
    from pointslot_amd._lib import PointslotError
    r = dict(share_id=[1, 2], share_words=[5, 5], share_score=[0.5, 0.4], min_common_words=1)
    assert kfdb.select(0, 0.0, r, {}) == [1, 2]
    assert kfdb.select(0, 0.0, dict(share_id=[], share_words=[], share_score=[], min_common_words=0), {}) == []
    with pytest.raises(PointslotError):
        kfdb.select(2, 0.0, r, {})
