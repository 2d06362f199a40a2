"""The comparisons of the mapping and place-recognition GPU tests (tests/test_{tri,bow,kfsearch,kfdb}_gpu.py), importable: the
randomised sweeps (tools/stress_{tri,bow,kfdb,kfsearch}.py) and tests/test_sweep_cases_cpu.py, which checks that each of them
notices one changed element, use the same functions.  Integers identical; x3d bit-equal for the stereo kinds and within one float32
ulp per coordinate for the linear triangulation; BowVector values within bow_cases.bow_val_bound(n); database scores bytewise.
Every function raises AssertionError on the first difference.  Test infrastructure, no GPU code."""
import numpy as np

import bow_cases
import tri_second_opinion as tri_so

F32 = np.float32
KF_KEYS = {0: ("match_of_train",), 1: ("best_idx", "best_dist"), 2: ("match_of_train",)}
SIM3_KEYS = ("match12", "match1", "match2")


def ulps(a, b):
    """distance in float32 steps (both finite, same sign or zero)"""
    ia, ib = a.astype(F32).view(np.int32).astype(np.int64), b.astype(F32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia); ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def tri_status_name(code):
    from pointslot_amd.matcher import TRI_STATUS
    return TRI_STATUS[int(code)] if int(code) < len(TRI_STATUS) else int(code)


def check_tri(got, ref, what=""):
    assert np.array_equal(got["match"], ref["match"]), (what, np.argwhere(got["match"] != ref["match"])[:5])
    assert np.array_equal(got["nmatches"], ref["nmatches"]), (what, got["nmatches"], ref["nmatches"])
    assert got["nnew"] == ref["nnew"], (what, got["nnew"], ref["nnew"])
    if "status" not in ref:
        assert "status" not in got
        return
    diff = np.argwhere(got["status"] != ref["status"])
    assert not len(diff), (what, [(tuple(d), tri_status_name(got["status"][tuple(d)]), tri_status_name(ref["status"][tuple(d)])) for d in diff[:5]])
    for p in ref["pairs"]:
        if p["kind"] == "none" or p["status"] == tri_so.W_ZERO or ref["match"][p["i"], p["idx1"]] < 0:
            continue
        g, r = got["x3d"][p["i"], p["idx1"]], ref["x3d"][p["i"], p["idx1"]]
        if p["kind"] == "svd":
            assert ulps(g, r).max() <= 1, (what, p, g, r)
        else:
            assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), (what, p, g, r)


def check_transform(got, ref, n, what=""):
    word, node, ids, vals = ref
    assert not got["failed"]
    assert np.array_equal(got["word"], word), (what, np.argwhere(got["word"] != word)[:5].ravel())
    assert np.array_equal(got["node"], node), (what, np.argwhere(got["node"] != node)[:5].ravel())
    assert len(got["bow_id"]) == len(ids) and np.array_equal(got["bow_id"], ids), what
    if len(ids):
        rel = np.abs(got["bow_val"] - vals) / np.abs(vals)
        assert rel.max() <= bow_cases.bow_val_bound(n), (what, rel.max(), bow_cases.bow_val_bound(n))


def check_bow_search(got, ref, what=""):
    """(nmatches, match) of ps_search_by_bow against search_by_bow's"""
    assert np.array_equal(got[1], ref[1]), (what, np.argwhere(got[1] != ref[1])[:5].ravel())
    assert got[0] == ref[0], (what, got[0], ref[0])


def check_kf(got, ref, mode, what=""):
    for key in KF_KEYS[mode]:
        assert np.array_equal(got[key], ref[key]), (what, key, np.argwhere(got[key] != ref[key])[:5].ravel(), got[key][got[key] != ref[key]][:5], ref[key][got[key] != ref[key]][:5])
    assert got["nmatches"] == ref["nmatches"], (what, got["nmatches"], ref["nmatches"])


def check_sim3(got, ref, what=""):
    for key in SIM3_KEYS:
        assert np.array_equal(got[key], ref[key]), (what, key, np.argwhere(got[key] != ref[key])[:5].ravel())
    assert got["nfound"] == ref["nfound"], (what, got["nfound"], ref["nfound"])


def check_kfdb_query(got, want, where=""):
    assert [int(x) for x in got["share_id"]] == [int(x) for x in want["share_id"]], where
    assert np.array_equal(got["share_words"], want["share_words"]), where
    assert got["share_score"].dtype == F32 and got["share_score"].tobytes() == want["share_score"].tobytes(), where
    assert got["min_common_words"] == want["min_common_words"], where
    assert got["candidates"] == want["candidates"], where


def check_kfdb_score(got, want, where=""):
    """ps_kfdb_score against the sequential double sum: double bits"""
    assert got.dtype == np.float64 and got.tobytes() == np.asarray(want, np.float64).tobytes(), where


def play_kfdb_device(db, case):
    """a kfdb_cases script on a device database: one result per query (and per ("score", bow, ids) op a dict(scores=...)), in order"""
    from pointslot_amd import kfdb
    out = []
    for op in case["ops"]:
        if op[0] == "add":
            assert all(db.add(op[1], [case["kfs"][i] for i in op[1]]))
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "score":
            out.append(dict(scores=db.score(op[1], op[2])))
        else:
            res = db.query([dict(bow=q["bow"], mode=q["mode"], excluded=q["connected"]) for q in op[1]])
            for q, r in zip(op[1], res):
                out.append(dict(r, candidates=kfdb.select(q["mode"], q["min_score"], r, case["neigh"])))
    return out
