"""CPU checks on the randomised sweeps of the mapping and place-recognition calls (tests/sweep_cases.py), under the very seeds and
budgets tests/test_random_sweeps_gpu.py runs tools/stress_{tri,bow,kfdb,kfsearch}.py with: the input conditions of the comparisons
hold for every problem (nothing is excluded), the sweeps reach what they are for, and the comparison helpers
(tests/parity_checks.py) notice one changed element of the second opinion's own answer."""
import numpy as np
import pytest

import bow_second_opinion as bow_so
import parity_checks as pc
import sweep_cases as sc
import tri_second_opinion as tri_so

F32 = np.float32


def _sweep(family):
    return sc.calls(family, *sc.COMMITTED[family]), sc.references(family, *sc.COMMITTED[family])


def test_the_gpu_suite_runs_the_committed_seeds():
    import test_random_sweeps_gpu as t
    for family, (seed, budget) in sc.COMMITTED.items():
        # (the matchers' committed scenes are the --cases mode of the tool that also keeps its older random scenes)
        tool, mode = ("stress_matchers.py", ["--cases"]) if family == "match" else ("stress_%s.py" % family, [])
        for rows in (t.SWEEPS, t.POISONED):                       # once plain, once with poisoned device memory
            assert [s[1] for s in rows if s[0] == tool and (not mode or s[1][:1] == mode)] == [mode + [str(seed), str(budget)]], family


def test_same_seed_same_bytes():
    for family in ("tri", "kfsearch"):
        seed, _ = sc.COMMITTED[family]
        a, b = sc._FAMILIES[family](seed, 6), sc._FAMILIES[family](seed, 6)
        for ca, cb in zip(a, b):
            for pa, pb in zip(ca["problems"], cb["problems"]):
                ka = pa["kf1"] if "kf1" in pa else pa["train"]
                kb = pb["kf1"] if "kf1" in pb else pb["train"]
                assert ka["desc"].tobytes() == kb["desc"].tobytes() and ka["x"].tobytes() == kb["x"].tobytes()


# ---- input conditions ------------------------------------------------------------------------------------------------------------
def test_tri_input_condition():
    """every triangulated pair of the committed run is stable and has sigma1 / sigma3 <= 1e5: no problem is skipped"""
    calls, refs = _sweep("tri")
    npairs = 0
    for c, rs in zip(calls, refs):
        for p, r in zip(c["problems"], rs):
            bad = sc.tri_bad_pairs(r)
            assert not bad, (p["settings"], bad[:3])
            npairs += len(r["pairs"])
    assert npairs > 1000


def test_kfsearch_input_condition():
    """no predicted level of the committed run sits within 4 ulp of a boundary"""
    calls, refs = _sweep("kfsearch")
    levels = 0
    for c, rs in zip(calls, refs):
        for r in rs:
            bad, n = sc.level_violations(r)
            assert bad == 0
            levels += n
    assert levels > 5000


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def test_tri_coverage():
    calls, refs = _sweep("tri")
    assert sum(len(c["problems"]) for c in calls) == sc.COMMITTED["tri"][1]
    seen, kinds, blocked, long_node, k32 = set(), set(), 0, 0, 0
    for c, rs in zip(calls, refs):
        for p, r in zip(c["problems"], rs):
            seen |= set(r["status"].ravel().tolist())
            kinds |= {q["kind"] for q in r["pairs"]}
            k32 += len(p["kf2"]) == 32
            long_node = max([long_node] + [int(np.bincount(kf["node"][kf["node"] >= 0] % 1000).max()) for kf in p["kf2"] if (kf["node"] >= 0).any()])
            if p["chain"]:
                free = p["kf1"]["occupied"] == 0
                for i in range(1, len(p["kf2"])):
                    blocked += int(((r["status"][i] == tri_so.OCCUPIED) & free & (r["status"][:i] == tri_so.CREATED).any(axis=0)).sum())
    assert {0, 1, 2, 3, 5, 7, 8, 10, 11} <= seen, seen
    assert {"svd", "stereo1", "stereo2"} <= kinds
    assert long_node > 64 and blocked >= 5 and k32 == 1
    assert any(len(c["problems"]) > 1 and len({len(p["kf1"]["node"]) for p in c["problems"]}) > 1 for c in calls)
    assert any(any(c["from_frame"]) for c in calls) and {len(p["kf1"]["node"]) for c in calls for p in c["problems"]} >= {1, 257, 513, 1100}


def _longest_run(words):
    w = np.sort(words[words >= 0])
    if not len(w):
        return 0
    edges = np.flatnonzero(np.concatenate([[True], w[1:] != w[:-1], [True]]))
    return int(np.diff(edges).max())


def test_bow_coverage():
    calls, refs = _sweep("bow")
    distinct, run, weightings, trees = 0, 0, set(), set()
    taken = ratio = 0
    for c, rs in zip(calls, refs):
        if c["kind"] == "transform":
            trees.add(c["tree"])
            weightings.add(sc.bow_vocabulary(sc.COMMITTED["bow"][0], *c["tree"])["weighting"])
            for f, (word, node, ids, vals) in zip(c["frames"], rs):
                if len(f) >= 1025:
                    distinct = max(distinct, len(ids))
                    run = max(run, _longest_run(word))
        else:
            for p, (n, match) in zip(c["problems"], rs):
                args = (p["a"], p["b"], p["mode"])
                taken += int((bow_so.search_by_bow(*args, p["nn_ratio"], p["check_orientation"], skip_rule=False)[1] != match).sum())
                ratio += int((bow_so.search_by_bow(*args, 1.0, p["check_orientation"])[1] != match).sum())
    assert distinct > 1000 and run > 256, (distinct, run)
    assert taken >= 20 and ratio >= 20, (taken, ratio)
    assert weightings == {0, 1, 2, 3} and len(trees) >= 4
    big = sc.bow_vocabulary(sc.COMMITTED["bow"][0], *sc.BOW_BIG)
    assert int((big["is_leaf"] != 0).sum()) >= 10 ** 4
    assert [c["kind"] for c in calls[:4]] == ["transform", "search", "transform", "search"]
    assert any(len(c["problems"]) % 4 for c in calls if c["kind"] == "search")


def test_kfdb_coverage():
    calls, refs = _sweep("kfdb")
    stale, spw, high_mod = 0, set(), set()
    for case, rs in zip(calls, refs):
        stale += sum(r["trace"]["stale_reads"] for r in rs if "trace" in r)
        for nq, high in sc.kfdb_high(case):
            spw.add(min(4, max(1, nq * high // 4096)))
            high_mod.add(high % 4)
    lengths = {len(b[0]) for b in calls[0]["kfs"].values()}
    assert set(sc.KFDB_STORED) <= lengths
    assert stale >= 1 and {1, 2, 3} <= spw and high_mod - {0}, (stale, spw, high_mod)
    ops = [op[0] for op in calls[0]["ops"]]
    assert {"add", "erase", "clear", "query", "score"} <= set(ops)
    sizes = [len(op[1]) for case in calls for op in case["ops"] if op[0] == "query"]
    assert 4 in sizes and 6 in sizes and max(sizes) <= 8
    asked = [q for op in calls[0]["ops"] if op[0] == "query" for q in op[1]]
    assert {q["mode"] for q in asked} == {0, 1} and any(q["connected"] for q in asked) and any(len(q["bow"][0]) == 2000 for q in asked)
    assert sum(len(r["share_id"]) > 0 and len(r["candidates"]) > 0 for r in refs[0] if "share_id" in r) >= 5


def test_kfsearch_coverage():
    calls, refs = _sweep("kfsearch")
    modes, mixed, reset, high, sim3_high, gates = set(), 0, 0, 0, 0, set()
    for c, rs in zip(calls, refs):
        if c["kind"] == "sim3":
            for p, r in zip(c["problems"], rs):
                sim3_high += int((r["match12"] >= 4096).sum()) + int((np.flatnonzero(r["match12"] >= 0) >= 4096).sum())
            continue
        over = [("dense" in p) and sc.takeable_bound(p, r, True) > sc.KS_CAP for p, r in zip(c["problems"], rs)]
        under = [("dense" not in p) and sc.takeable_bound(p, r, False) <= sc.KS_CAP for p, r in zip(c["problems"], rs)]
        assert all(o or u for o, u in zip(over, under))           # every problem is known to be on one side
        mixed += any(over) and any(under)
        for p, r in zip(c["problems"], rs):
            modes.add(p["mode"])
            gates |= set(r["gate"])
            if p["mode"] == 1:
                high += int((r["best_idx"] >= 4096).sum())
            else:
                reset += int((r["match_of_train"] == -2).sum())
                high += int((np.flatnonzero(r["match_of_train"] >= 0) >= 4096).sum())
    assert modes == {0, 1, 2} and mixed >= 2 and reset >= 5 and high >= 2 and sim3_high >= 1, (modes, mixed, reset, high, sim3_high)
    assert {"invalid", "depth", "image", "distance", "angle", "empty", "nomatch", "match"} <= gates
    assert any(any(c["from_frame"]) for c in calls if c["kind"] == "kf")


# ---- the comparison helpers notice one changed element --------------------------------------------------------------------------------
def _first(calls, refs, want):
    for c, rs in zip(calls, refs):
        for j, r in enumerate(rs):
            if want(c, j, r):
                return c, j, r
    raise AssertionError("no such result in the sweep")


def _next(v, k=1):
    for _ in range(k):
        v = np.nextafter(v, v.dtype.type(np.inf))
    return v


def test_tri_checker_sensitivity():
    calls, refs = _sweep("tri")
    _, _, ref = _first(calls, refs, lambda c, j, r: {"svd", "stereo1"} <= {p["kind"] for p in r["pairs"] if p["status"] == 0})
    pc.check_tri(ref, ref)
    m = dict(ref, match=ref["match"].copy()); m["match"][tuple(np.argwhere(ref["match"] >= 0)[0])] += 1
    s = dict(ref, status=ref["status"].copy()); s["status"].flat[0] ^= 1
    changed = [m, s, dict(ref, nnew=ref["nnew"] + 1)]
    for kind, steps in (("svd", 2), ("stereo1", 1)):          # one coordinate: 2 ulp where 1 is allowed, 1 ulp where none is
        p = [q for q in ref["pairs"] if q["kind"] == kind and q["status"] == 0][0]
        x = dict(ref, x3d=ref["x3d"].copy())
        x["x3d"][p["i"], p["idx1"], 1] = _next(x["x3d"][p["i"], p["idx1"], 1], steps)
        changed.append(x)
    for got in changed:
        with pytest.raises(AssertionError):
            pc.check_tri(got, ref)
    p = [q for q in ref["pairs"] if q["kind"] == "svd" and q["status"] == 0][0]
    x = dict(ref, x3d=ref["x3d"].copy())
    x["x3d"][p["i"], p["idx1"], 1] = _next(x["x3d"][p["i"], p["idx1"], 1], 1)
    pc.check_tri(x, ref)                                        # ... and one ulp on a triangulated point is inside the bound


def test_bow_checker_sensitivity():
    calls, refs = _sweep("bow")
    c, j, (word, node, ids, vals) = _first(calls, refs, lambda c, j, r: c["kind"] == "transform" and len(r[2]) > 100)
    n = len(c["frames"][j])
    good = dict(word=word, node=node, bow_id=ids, bow_val=vals, failed=False)
    pc.check_transform(good, (word, node, ids, vals), n)
    w2 = word.copy(); w2[0] += 1
    n2 = node.copy(); n2[-1] += 1
    i2 = ids.copy(); i2[len(ids) // 2] += 1 if ids[len(ids) // 2] + 1 not in ids else 2
    v2 = vals.copy(); v2[3] = v2[3] * (1 + 2 * (n + 2) * 2.0 ** -52)
    for got in (dict(good, word=w2), dict(good, node=n2), dict(good, bow_id=i2), dict(good, bow_id=ids[:-1], bow_val=vals[:-1]), dict(good, bow_val=v2)):
        with pytest.raises(AssertionError):
            pc.check_transform(got, (word, node, ids, vals), n)
    c, j, (nm, match) = _first(calls, refs, lambda c, j, r: c["kind"] == "search" and r[0] > 10)
    pc.check_bow_search((nm, match), (nm, match))
    m2 = match.copy(); m2[np.flatnonzero(match >= 0)[0]] = -1
    for got in ((nm, m2), (nm - 1, match)):
        with pytest.raises(AssertionError):
            pc.check_bow_search(got, (nm, match))


def test_kfdb_checker_sensitivity():
    calls, refs = _sweep("kfdb")
    _, _, ref = _first(calls, refs, lambda c, j, r: "share_id" in r and len(r["share_id"]) > 3 and len(r["candidates"]) > 0 and (r["share_score"] > 0).any())
    pc.check_kfdb_query(ref, ref)
    k = int(np.flatnonzero(ref["share_score"] > 0)[0])
    sco = ref["share_score"].copy(); sco[k] = _next(sco[k])
    sid = ref["share_id"].copy(); sid[[0, 1]] = sid[[1, 0]]
    sw = ref["share_words"].copy(); sw[-1] += 1
    for got in (dict(ref, share_score=sco), dict(ref, share_id=sid), dict(ref, share_words=sw), dict(ref, min_common_words=ref["min_common_words"] + 1),
                dict(ref, candidates=ref["candidates"][:-1])):
        with pytest.raises(AssertionError):
            pc.check_kfdb_query(got, ref)
    _, _, ref = _first(calls, refs, lambda c, j, r: "scores" in r and (r["scores"] > 0).any())
    pc.check_kfdb_score(ref["scores"], ref["scores"])
    s2 = ref["scores"].copy(); k = int(np.flatnonzero(s2 > 0)[0]); s2[k] = _next(s2[k])
    with pytest.raises(AssertionError):
        pc.check_kfdb_score(s2, ref["scores"])


def test_kfsearch_checker_sensitivity():
    calls, refs = _sweep("kfsearch")
    for mode in (0, 1, 2):
        c, j, ref = _first(calls, refs, lambda c, j, r: c["kind"] == "kf" and r["nmatches"] > 3 and c["problems"][j]["mode"] == mode)
        pc.check_kf(ref, ref, mode)
        key = pc.KF_KEYS[mode][0]
        a = ref[key].copy(); a[np.flatnonzero(a >= 0)[0]] += 1
        changed = [dict(ref, **{key: a}), dict(ref, nmatches=ref["nmatches"] - 1)]
        if mode == 1:
            b = ref["best_dist"].copy(); b[0] -= 1
            changed.append(dict(ref, best_dist=b))
        for got in changed:
            with pytest.raises(AssertionError):
                pc.check_kf(got, ref, mode)
    _, _, ref = _first(calls, refs, lambda c, j, r: c["kind"] == "sim3" and r["nfound"] > 3)
    pc.check_sim3(ref, ref)
    for key in pc.SIM3_KEYS:
        a = ref[key].copy(); a[np.flatnonzero(a >= 0)[0]] = -1
        with pytest.raises(AssertionError):
            pc.check_sim3(dict(ref, **{key: a}), ref)
    with pytest.raises(AssertionError):
        pc.check_sim3(dict(ref, nfound=ref["nfound"] + 1), ref)
