"""ps_kf_search and ps_search_by_sim3 on the GPU against the numpy second opinion (tests/kfsearch_second_opinion.py) on the seeded
cases of tests/kfsearch_cases.py.  Every output is an integer and must be identical: match_of_train, nmatches, best_idx, best_dist,
match12, nfound and the raw match1 / match2.  There is no tolerance in this feature; tests/test_kfsearch_cpu.py checks on the CPU
that no predicted level of any case sits within 4 ulp of a boundary."""
import numpy as np
import pytest

import kfsearch_cases as kc
import parity_checks
from pointslot_amd import _lib
from pointslot_amd.frame import DeviceFrame
from pointslot_amd.matcher import ORBmatcher

pytestmark = pytest.mark.gpu
KF_KEYS, SIM3_KEYS = parity_checks.KF_KEYS, parity_checks.SIM3_KEYS


@pytest.fixture(scope="module")
def matcher():
    m = ORBmatcher(0.6, True)
    yield m
    m.close()


_check_kf, _check_sim3 = parity_checks.check_kf, parity_checks.check_sim3


def _run(matcher, name):
    return matcher.KfSearch([kc.problem(name)])[0]


@pytest.mark.parametrize("name", ["main_0", "main_1", "main_2", "main_2_64", "rot13"])
def test_members_equal_the_second_opinion(matcher, name):
    pr, ref = kc.problem(name), kc.reference(name)
    assert ref["nmatches"] > 50
    _check_kf(_run(matcher, name), ref, pr["mode"], name)


@pytest.mark.parametrize("name", ["limit_0", "limit_2"])
def test_searched_side_at_the_feature_limit(matcher, name):
    """8191 searched features in a random order and 3000 points: matches at indices on both sides of 4096"""
    pr, ref = kc.problem(name), kc.reference(name)
    at = np.flatnonzero(ref["match_of_train"] >= 0)
    assert len(pr["train"]["x"]) == 8191 and (at >= 4096).sum() > 200 and (at < 4096).sum() > 200
    _check_kf(_run(matcher, name), ref, pr["mode"], name)


def test_reference_named_entries(matcher):
    ref = kc.reference("main_0")
    n, m = matcher.SearchByProjectionSim3([kc.problem("main_0")])[0]
    assert n == ref["nmatches"] and np.array_equal(m, ref["match_of_train"])
    ref = kc.reference("main_1")
    bi, bd = matcher.FuseSim3([kc.problem("main_1")])[0]
    assert np.array_equal(bi, ref["best_idx"]) and np.array_equal(bd, ref["best_dist"])
    ref = kc.reference("main_2")
    n, m = matcher.SearchByProjectionKeyFrame([kc.problem("main_2")])[0]
    assert n == ref["nmatches"] and np.array_equal(m, ref["match_of_train"]) and (m == -2).any()


@pytest.mark.parametrize("mode", [0, 2])
def test_contention(matcher, mode):
    name = "contention_%d" % mode
    pr, got = kc.problem(name), _run(matcher, name)
    for slot, point in pr["expect"].items():
        assert got["match_of_train"][slot] == point, (slot, point)
    _check_kf(got, kc.reference(name), mode, name)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_first_in_traversal_order_wins(matcher, mode):
    name = "tie_%d" % mode
    pr, got = kc.problem(name), _run(matcher, name)
    for p, left, right in pr["expect_tie"]:
        if mode == 1:
            assert got["best_idx"][p] == left
        else:
            assert got["match_of_train"][left] == p and got["match_of_train"][right] == -1
    _check_kf(got, kc.reference(name), mode, name)


@pytest.mark.parametrize("name", ["behind_2", "behind_0", "edge_0", "edge_1", "edge_2"])
def test_depth_sign_and_bounds_as_written(matcher, name):
    pr = kc.problem(name)
    got = _run(matcher, name)
    _check_kf(got, kc.reference(name), pr["mode"], name)
    assert got["nmatches"] == (1 if name in ("behind_2", "edge_2") else 0)


@pytest.mark.parametrize("mode", [0, 2])
def test_wide_rerun(matcher, mode):
    name = "wide_%d" % mode
    _check_kf(_run(matcher, name), kc.reference(name), mode, name)
    # ... beside problems that stay in the everyday store, in either order
    got = matcher.KfSearch([kc.problem("batch_00"), kc.problem(name), kc.problem("batch_02")])
    _check_kf(got[1], kc.reference(name), mode, name)
    _check_kf(got[0], kc.reference("batch_00"), 0, "beside the wide one")
    _check_kf(got[2], kc.reference("batch_02"), 2, "beside the wide one")


@pytest.mark.parametrize("name", ["empty_nq_0", "empty_nq_1", "empty_n_2", "empty_n_1"])
def test_empty_sides(matcher, name):
    pr = kc.problem(name)
    _check_kf(_run(matcher, name), kc.reference(name), pr["mode"], name)
    assert matcher.KfSearch([]) == [] and matcher.SearchBySim3([]) == []


def test_capacity_fails_that_problem_alone(matcher):
    probs = kc.over()
    with pytest.raises(_lib.PointslotError) as e:
        matcher.KfSearch(probs)
    assert e.value.code == _lib.PS_ERR_CAPACITY
    got = matcher.KfSearch(probs, partial_ok=True)
    assert got[1]["nmatches"] == -1 and (got[1]["match_of_train"] == -3).all()       # outputs untouched
    import kfsearch_second_opinion as so
    _check_kf(got[0], so.run(probs[0]), 0, "beside a problem beyond the limits")
    _check_kf(got[2], so.run(probs[2]), 2, "beside a problem beyond the limits")


def test_bad_arguments(matcher):
    bad = dict(kc.problem("batch_00"), mode=3)
    with pytest.raises(_lib.PointslotError) as e:
        matcher.KfSearch([bad])
    assert e.value.code == _lib.PS_ERR_INVALID
    bad = dict(kc.problem("batch_02"), th_dist=300)
    with pytest.raises(_lib.PointslotError) as e:
        matcher.KfSearch([bad])
    assert e.value.code == _lib.PS_ERR_INVALID


def test_batch_equals_single_calls(matcher):
    batch = matcher.KfSearch([kc.problem(n) for n in kc.BATCH])
    for name, got in zip(kc.BATCH, batch):
        mode = kc.problem(name)["mode"]
        _check_kf(got, kc.reference(name), mode, name)
        single = _run(matcher, name)
        for key in KF_KEYS[mode]:
            assert np.array_equal(got[key], single[key]), (name, key)
        assert got["nmatches"] == single["nmatches"]


def test_same_problem_twice_on_one_handle(matcher):
    for name in ("main_0", "main_2", "contention_2", "wide_0"):
        a, b = _run(matcher, name), _run(matcher, name)
        assert np.array_equal(a["match_of_train"], b["match_of_train"]) and a["nmatches"] == b["nmatches"], name
    twice = matcher.KfSearch([kc.problem("main_0"), kc.problem("main_0")])
    assert np.array_equal(twice[0]["match_of_train"], twice[1]["match_of_train"])
    assert matcher.last_kernel_ms() > 0


def _published(train):
    f = DeviceFrame(len(train["x"]) + 5)
    f.publish(train, None, train["desc"], train["grid"])
    return f


def test_searched_side_from_a_frame_handle(matcher):
    """one handle backs several problems (a relocalising frame is searched once per candidate keyframe), mixed with host-side problems"""
    base = kc.problem("main_2")
    frame = _published(base["train"])
    others = []
    for seed in (3, 4):          # other candidate keyframes: the same frame, other points
        rng = np.random.RandomState(seed)
        keep = rng.rand(len(base["query"]["valid"])) < 0.6
        others.append(dict(base, query=dict(base["query"], valid=(base["query"]["valid"] * keep).astype(np.uint8))))
    plain = matcher.KfSearch([base] + others + [kc.problem("main_1")])
    via = [dict(p, train=dict(frame=frame, occupied=p["train"]["occupied"])) for p in [base] + others]
    got = matcher.KfSearch(via + [kc.problem("main_1")])
    for g, p in zip(got[:3], plain[:3]):
        assert np.array_equal(g["match_of_train"], p["match_of_train"]) and g["nmatches"] == p["nmatches"]
    _check_kf(got[0], kc.reference("main_2"), 2, "through the handle")
    again = matcher.KfSearch(via + [kc.problem("main_1")])     # the same problems once more on the same handles
    for g, a in zip(got[:3], again[:3]):
        assert np.array_equal(g["match_of_train"], a["match_of_train"]) and g["nmatches"] == a["nmatches"]
    _check_kf(got[3], kc.reference("main_1"), 1, "host-side beside handles")
    f1 = _published(kc.problem("main_1")["train"])
    fuse = dict(kc.problem("main_1"), train=dict(frame=f1))
    _check_kf(matcher.KfSearch([fuse])[0], kc.reference("main_1"), 1, "fuse through the handle")
    short = dict(base, train=dict(frame=frame, occupied=base["train"]["occupied"][:-1]))
    with pytest.raises(ValueError):
        matcher.KfSearch([short])
    frame.close(); f1.close()


def test_kf_search_mixed_batch(matcher):
    """One call with a frame-backed problem (mode 0), a host-backed one (mode 1) and a frame-backed one whose frame is empty (mode 2):
    some searched sides are staged on the device, so nothing of the upload may be left out.  65 features and 5 points each."""
    probs = [kc.problem(n) for n in kc.MIXED]
    assert [p["mode"] for p in probs] == [0, 1, 2] and [len(p["train"]["x"]) for p in probs] == [65, 65, 0]
    assert all(len(p["query"]["valid"]) == 5 for p in probs) and kc.reference("mixed_0")["nmatches"] > 0 and kc.reference("mixed_1")["nmatches"] > 0
    alone = [matcher.KfSearch([p])[0] for p in probs]
    frames = [_published(probs[0]["train"]), None, _published(probs[2]["train"])]
    via = [p if f is None else dict(p, train=dict(frame=f, occupied=p["train"]["occupied"])) for p, f in zip(probs, frames)]
    got = matcher.KfSearch(via)
    for name, p, g, a in zip(kc.MIXED, probs, got, alone):
        _check_kf(g, kc.reference(name), p["mode"], name)
        _check_kf(a, kc.reference(name), p["mode"], name + " alone")
        for key in KF_KEYS[p["mode"]]:
            assert np.array_equal(g[key], a[key]), (name, key)
    frames[0].close(); frames[2].close()


@pytest.mark.parametrize("name", sorted(kc.SIM3_BUILDERS))
def test_search_by_sim3_equals_the_second_opinion(matcher, name):
    _check_sim3(matcher.SearchBySim3([kc.problem(name)])[0], kc.reference(name), name)


def test_search_by_sim3_pairs(matcher):
    pr, ref = kc.problem("sim3_main_093"), kc.reference("sim3_main_093")
    got = matcher.SearchBySim3([pr])[0]
    assert got["nfound"] >= 50 and (got["match12"][pr["kf1"]["already"] > 0] == -1).all()
    assert ((got["match1"] >= 0) & (got["match12"] < 0)).sum() >= 10           # matched one way only
    pt, gt = kc.problem("sim3_tie"), matcher.SearchBySim3([kc.problem("sim3_tie")])[0]
    for i1, left, right in pt["expect_tie"]:
        assert gt["match12"][i1] == left
    # the reference's own signature: keyframe 1's intrinsics serve both directions (keyframe 2 carries another fx)
    n, m12 = matcher.SearchBySim3(pr["kf1"], pr["kf2"], pr["matches12"], pr["s12"], pr["R12"], pr["t12"], pr["th"])
    assert n == ref["nfound"]
    want = pr["matches12"].copy()
    want[ref["match12"] >= 0] = ref["match12"][ref["match12"] >= 0]
    assert np.array_equal(m12, want) and (m12 >= 0).sum() == 40 + ref["nfound"]


def test_search_by_sim3_batch_and_frames(matcher):
    names = sorted(kc.SIM3_BUILDERS)
    batch = matcher.SearchBySim3([kc.problem(n) for n in names])
    for name, got in zip(names, batch):
        _check_sim3(got, kc.reference(name), name)
    pr = kc.problem("sim3_main")
    f1, f2 = _published(pr["kf1"]), _published(pr["kf2"])
    strip = lambda kf, f: dict({k: v for k, v in kf.items() if k not in ("x", "y", "octave", "angle", "desc", "cell_off", "cell_idx", "grid")}, frame=f)
    via = dict(pr, kf1=strip(pr["kf1"], f1), kf2=strip(pr["kf2"], f2))
    half = dict(pr, kf2=strip(pr["kf2"], f2))
    for got in matcher.SearchBySim3([via, pr, half]):
        _check_sim3(got, kc.reference("sim3_main"), "through frame handles")
    f1.close(); f2.close()
    big = kc.problem("sim3_small")
    n = 8192
    kf = dict(big["kf2"])
    for k in ("x", "y", "octave", "angle", "has_point", "min_dist", "max_dist", "already"):
        kf[k] = np.resize(kf[k], n)
    for k, w in (("desc", 32), ("point_desc", 32), ("pos", 3)):
        kf[k] = np.resize(kf[k], (n, w))
    from pointslot_amd.matcher import build_grid
    kf["cell_off"], kf["cell_idx"] = build_grid(kf["x"], kf["y"], *kf["grid"])
    got = matcher.SearchBySim3([dict(big, kf2=kf), kc.problem("sim3_small")], partial_ok=True)
    assert got[0]["nfound"] == -1 and (got[0]["match12"] == -3).all()
    _check_sim3(got[1], kc.reference("sim3_small"), "beside a problem beyond the limits")
