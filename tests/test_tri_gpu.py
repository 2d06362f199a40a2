"""ps_create_new_map_points on the GPU against the numpy second opinion (tests/tri_second_opinion.py) on the seeded cases of
tests/tri_cases.py: match, nmatches, status and nnew identical; x3d within one float32 ulp per coordinate where the point comes
from the linear triangulation (two FP64 null vectors of a well-conditioned A, tests/test_tri_cpu.py checks the condition) and
bit-equal where it comes from KeyFrame::UnprojectStereo."""
import numpy as np
import pytest

import parity_checks
import tri_cases
import tri_second_opinion as so
from pointslot_amd import _lib, keyframes
from pointslot_amd.frame import DeviceFrame
from pointslot_amd.matcher import ORBmatcher

pytestmark = pytest.mark.gpu
F32 = np.float32
GRID = (0.0, 0.0, F32(64) / F32(1241), F32(48) / F32(376))


@pytest.fixture(scope="module")
def matcher():
    m = ORBmatcher(0.6, False)
    yield m
    m.close()


_ulps, _check, so_name = parity_checks.ulps, parity_checks.check_tri, parity_checks.tri_status_name


def _run(matcher, name):
    return matcher.CreateNewMapPoints([tri_cases.problem(name)])[0]


@pytest.mark.parametrize("name", ["main", "noisy", "raw", "no_orientation", "only_stereo_tri"])
def test_search_triangulation_and_chain_equal_the_second_opinion(matcher, name):
    ref = tri_cases.reference(name)
    assert ref["nnew"] > 20
    _check(_run(matcher, name), ref, name)


@pytest.mark.parametrize("name", ["search_00", "search_01", "search_10", "search_11"])
def test_search_alone(matcher, name):
    pr, ref = tri_cases.problem(name), tri_cases.reference(name)
    _check(_run(matcher, name), ref, name)
    # ... and through the reference-shaped entry, neighbour by neighbour
    m = ORBmatcher(0.6, bool(pr["check_orientation"]))
    for i, kf2 in enumerate(pr["kf2"]):
        n, pairs = m.SearchForTriangulation(pr["kf1"], kf2, pr["f12"][i], bool(pr["only_stereo"]))
        assert n == ref["nmatches"][i] and pairs == [(int(j), int(ref["match"][i, j])) for j in np.nonzero(ref["match"][i] >= 0)[0]]
    m.close()


def test_equal_distances_go_to_the_highest_index(matcher):
    pr, got = tri_cases.problem("tie"), _run(matcher, "tie")
    for (i, idx1), (low, high) in pr["expect_tie"].items():
        assert got["match"][i, idx1] == high
    _check(got, tri_cases.reference("tie"), "tie")


def test_two_features_may_choose_the_same_partner(matcher):
    pr, got = tri_cases.problem("shared_partner"), _run(matcher, "shared_partner")
    for s, d in pr["expect_shared"]:
        assert got["match"][0, s] == got["match"][0, d] >= 0
    _check(got, tri_cases.reference("shared_partner"), "shared_partner")


def test_node_lists_longer_than_a_wave(matcher):
    _check(_run(matcher, "long_node"), tri_cases.reference("long_node"), "long_node")


def test_features_in_no_node_match_nothing(matcher):
    pr, got = tri_cases.problem("main"), _run(matcher, "main")
    none = pr["kf1"]["node"] < 0
    assert none.any() and (got["match"][:, none] == -1).all() and np.isin(got["status"][:, none], (so.NO_MATCH, so.OCCUPIED)).all()


def test_mono_pair_inside_the_epipole_disc(matcher):
    for name, matched in (("epipole_mono", False), ("epipole_stereo1", True)):
        pr, got = tri_cases.problem(name), _run(matcher, name)
        for idx1, idx2 in pr["expect_epipole"]:
            assert got["match"][0, idx1] == (idx2 if matched else -1), (name, idx1)
        _check(got, tri_cases.reference(name), name)


def test_chain(matcher):
    on, off = _run(matcher, "chain_on"), _run(matcher, "chain_off")
    _check(on, tri_cases.reference("chain_on"), "chain_on")
    _check(off, tri_cases.reference("chain_off"), "chain_off")
    again = [(i, j) for i in (1, 2) for j in range(on["match"].shape[1]) if off["match"][i, j] >= 0 and (on["status"][:i, j] == 0).any()]
    assert len(again) >= 5 and all(on["status"][i, j] == so.OCCUPIED and on["match"][i, j] == -1 for i, j in again)
    assert on["nmatches"][1] < off["nmatches"][1]     # the rotation histogram of neighbour 1 does not count them


def test_neighbour_below_the_baseline(matcher):
    got = _run(matcher, "baseline")
    assert (got["status"][1] == so.SKIPPED).all() and got["nmatches"][1] == 0 and (got["match"][1] == -1).all()
    _check(got, tri_cases.reference("baseline"), "baseline")


@pytest.mark.parametrize("name", ["empty_kf1", "empty_neighbour", "no_neighbours"])
def test_empty_sides(matcher, name):
    _check(_run(matcher, name), tri_cases.reference(name), name)


def test_32_neighbours(matcher):
    _check(_run(matcher, "k32"), tri_cases.reference("k32"), "k32")


def test_batch_equals_single_calls(matcher):
    batch = matcher.CreateNewMapPoints([tri_cases.problem(n) for n in tri_cases.BATCH])
    for name, got in zip(tri_cases.BATCH, batch):
        _check(got, tri_cases.reference(name), name)
        single = _run(matcher, name)
        for key in ("match", "nmatches", "status", "x3d"):
            assert np.array_equal(got[key].view(np.uint8), single[key].view(np.uint8)), (name, key)
        assert got["nnew"] == single["nnew"]


def test_keyframe_1_from_a_frame_handle(matcher):
    pr = tri_cases.problem("raw")
    plain = matcher.CreateNewMapPoints([pr])[0]
    kf1 = pr["kf1"]
    n = len(kf1["node"])
    frame = DeviceFrame(n + 7)
    frame.publish(kf1, kf1["u_right"], kf1["desc"], GRID)
    held = {k: kf1[k] for k in ("depth", "node", "occupied", "x_raw", "y_raw", "R", "t", "ow", "K8", "scale_factors", "level_sigma2")}
    held["frame"] = frame
    via = dict(pr); via["kf1"] = held
    got = matcher.CreateNewMapPoints([via, pr])          # a batch may mix both kinds
    for g in got:
        for key in ("match", "nmatches", "status", "x3d"):
            assert np.array_equal(g[key].view(np.uint8), plain[key].view(np.uint8)), key
        assert g["nnew"] == plain["nnew"]
    _check(got[0], tri_cases.reference("raw"), "raw through the handle")
    short = dict(held); short.update({k: held[k][:-1] for k in ("depth", "node", "occupied", "x_raw", "y_raw")})
    bad = dict(pr); bad["kf1"] = short
    with pytest.raises(_lib.PointslotError) as e:
        matcher.CreateNewMapPoints([bad])
    assert e.value.code == _lib.PS_ERR_INVALID
    frame.close()


def test_capacity_fails_that_problem_alone(matcher):
    big = keyframes.keyframe_set(41, n_kf=2, sizes=[8192, 40], flip_bits=0)
    ok = tri_cases.problem("limit_8191x40")              # keyframe_set(42, n_kf=2, sizes=[8191, 40], flip_bits=0), as before
    small = tri_cases.problem("batch_1")
    with pytest.raises(_lib.PointslotError) as e:
        matcher.CreateNewMapPoints([keyframes.problem_of(big), small])
    assert e.value.code == _lib.PS_ERR_CAPACITY
    got = matcher.CreateNewMapPoints([keyframes.problem_of(big), small, ok], partial_ok=True)
    assert got[0]["failed"] and not got[1]["failed"] and not got[2]["failed"]
    _check(got[1], tri_cases.reference("batch_1"), "beside a problem beyond the limits")
    assert got[2]["match"].shape == (1, 8191) and got[2]["nnew"] >= 0
    _check(got[2], tri_cases.reference("limit_8191x40"), "8191 features beside a problem beyond the limits")
    too_many = keyframes.tri_problem(43, k=33, n1=8, n2=8)
    with pytest.raises(_lib.PointslotError) as e:
        matcher.CreateNewMapPoints([too_many])
    assert e.value.code == _lib.PS_ERR_CAPACITY


def test_keyframes_at_the_feature_limit(matcher):
    """8191 x 8191 features, one neighbour, 200 nodes: 32 workgroups in y, every word of the occupied bitmap, 32 trips of the
    256-wide loops, matches on both sides of index 4096"""
    ref = tri_cases.reference("limit_8191x8191")
    assert (np.flatnonzero(ref["match"][0] >= 0) >= 4096).sum() > 100 and (ref["match"][0] >= 4096).sum() > 100 and ref["nnew"] > 100
    _check(_run(matcher, "limit_8191x8191"), ref, "limit_8191x8191")
