"""ps_bow_transform and ps_search_by_bow on the GPU against the second opinion (tests/bow_second_opinion.py) on the cases of
tests/bow_cases.py: word, node, the BowVector's ids and length, match and nmatches bit-equal; the BowVector's values within
(n + 2) 2^-52 relative (bow_cases.bow_val_bound: the one reorderable operation is the L1 sum)."""
import numpy as np
import pytest

import bow_cases
import parity_checks
import bow_second_opinion as so
from pointslot_amd import bow, keyframes
from pointslot_amd.matcher import ORBmatcher
from pointslot_amd.optimizer import Optimizer

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def matcher():
    m = ORBmatcher(0.6, True)
    yield m
    m.close()


_VOCABS = {}


def _device_vocabulary(name):
    if name not in _VOCABS:
        v = bow_cases.hand_vocabulary() if name == "hand" else bow_cases.vocabulary(name)
        _VOCABS[name] = bow.Vocabulary.from_arrays(**v)
    return _VOCABS[name]


_check_transform = parity_checks.check_transform


@pytest.mark.parametrize("weighting", [so.TF_IDF, so.TF, so.IDF, so.BINARY])
def test_transform_hand_built_vocabulary(matcher, weighting):
    voc = bow.Vocabulary.from_arrays(**bow_cases.hand_vocabulary(weighting))
    assert voc.info() == dict(k=3, L=3, nodes=25, words=17)
    raw = np.array(bow_cases.HAND_BOW_VALUES[weighting])
    levels = sorted(bow_cases.HAND_NODES)
    res = voc.transform([bow_cases.HAND_FEATURES] * len(levels), levels, matcher=matcher)
    for levelsup, r in zip(levels, res):
        assert r["word"].tolist() == bow_cases.HAND_WORDS
        assert r["node"].tolist() == bow_cases.HAND_NODES[levelsup], levelsup
        assert r["bow_id"].tolist() == bow_cases.HAND_BOW_IDS
        assert np.abs(r["bow_val"] - raw / raw.sum()).max() <= 9 * 2.0 ** -52
    voc.close()


@pytest.mark.parametrize("name", sorted(bow_cases.TRANSFORM_CASES))
def test_transform_seeded_vocabularies(matcher, name):
    case = bow_cases.TRANSFORM_CASES[name]
    voc = _device_vocabulary(name)
    v = bow_cases.vocabulary(name)
    assert voc.info() == dict(k=v["k"], L=v["L"], nodes=len(v["parent"]) + 1, words=int((v["is_leaf"] != 0).sum()))
    feats = bow_cases.transform_features(name)
    res = voc.transform([feats] * len(case["levelsup"]), list(case["levelsup"]), matcher=matcher)
    for levelsup, r in zip(case["levelsup"], res):
        _check_transform(r, bow_cases.transform_reference(name, levelsup), len(feats), (name, levelsup))


def test_transform_empty_and_single_and_unequal_batch(matcher):
    """n = 0, n = 1 and five frames of unequal sizes in one call: every frame equals its own second opinion"""
    name = "pruned_k3_L6"
    voc, ref_voc = _device_vocabulary(name), bow_cases.second_opinion_vocabulary(name)
    feats = bow_cases.transform_features(name)
    sizes = [0, 1, 17, 64, 33]
    frames = [feats[10:10 + s] for s in sizes]
    res = voc.transform(frames, 2, matcher=matcher)
    assert len(res[0]["word"]) == 0 and len(res[0]["bow_id"]) == 0 and not res[0]["failed"]
    for f, r in zip(frames, res):
        _check_transform(r, ref_voc.transform(f, 2), len(f), len(f))


def test_transform_vocabulary_loaded_from_a_file(matcher, tmp_path):
    name = "wide_k20_L2"
    v = bow_cases.vocabulary(name)
    path = str(tmp_path / "voc.bin")
    bow.Vocabulary.save_binary(path, v["k"], v["L"], v["weighting"], v["parent"], v["desc"], v["weight"], v["is_leaf"])
    voc = bow.Vocabulary.load(path)
    assert voc.info() == _device_vocabulary(name).info()
    feats = bow_cases.transform_features(name)
    _check_transform(voc.transform([feats], 1, matcher=matcher)[0], bow_cases.transform_reference(name, 1), len(feats), name)
    voc.close()
    with open(path, "r+b") as f:
        f.truncate(24 + 41 * 7 + 3)
    with pytest.raises(Exception) as e:
        bow.Vocabulary.load(path)
    assert e.value.code == -1


def test_vocabulary_create_rejects_what_the_reference_cannot_walk():
    v = bow_cases.hand_vocabulary()
    for change, what in (((4, 9), "forward parent"), ((5, 3), "leaf parent")):
        bad = dict(v, parent=v["parent"].copy())
        bad["parent"][change[0]] = change[1]
        with pytest.raises(Exception) as e:
            bow.Vocabulary.from_arrays(**bad)
        assert e.value.code == -1, what
    childless = dict(v, is_leaf=v["is_leaf"].copy())
    childless["is_leaf"][23] = 0                                   # node 24 becomes an inner node with no children
    with pytest.raises(Exception) as e:
        bow.Vocabulary.from_arrays(**childless)
    assert e.value.code == -1
    for kw in (dict(k=21), dict(L=11), dict(scoring=1), dict(weighting=4)):
        with pytest.raises(Exception) as e:
            bow.Vocabulary.from_arrays(**dict(v, **kw))
        assert e.value.code == -1, kw


def test_transform_beyond_the_limit_fails_alone(matcher):
    voc = _device_vocabulary("hand")
    big = np.tile(bow_cases.HAND_FEATURES, (1171, 1))[:8192]
    res = voc.transform([bow_cases.HAND_FEATURES, big, big[:8191]], 0, matcher=matcher, partial_ok=True)
    assert res[1]["failed"] and not res[0]["failed"] and not res[2]["failed"]
    assert res[0]["word"].tolist() == bow_cases.HAND_WORDS
    assert res[2]["word"].tolist() == (bow_cases.HAND_WORDS * 1171)[:8191]
    with pytest.raises(Exception) as e:
        voc.transform([big], 0, matcher=matcher)
    assert e.value.code == -3
    # ... and a frame AT the limit on a 10^4-word tree, value for value, beside one beyond it
    name = "limit_k10_L4"
    feats = bow_cases.transform_features(name)
    ref = bow_cases.transform_reference(name, 2)
    assert len(feats) == bow.MAX_N == 8191 and len(ref[2]) > 4096
    res = _device_vocabulary(name).transform([feats, np.concatenate([feats, feats[:1]]), feats[:100]], 2, matcher=matcher, partial_ok=True)
    assert res[1]["failed"]
    _check_transform(res[0], ref, len(feats), name)
    _check_transform(res[2], bow_cases.second_opinion_vocabulary(name).transform(feats[:100], 2), 100, name)


# ---- search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_search_hand_built_case(matcher, mode):
    a, b, want = bow_cases.hand_search()
    n, match = matcher.SearchByBoWBatch([dict(a=a, b=b, mode=mode, nn_ratio=0.9, check_orientation=1)])[0]
    expect = np.full(len(match), -1, np.int32)
    for i, v in want[mode].items():
        expect[i] = v
    assert match.tolist() == expect.tolist() and n == len(want[mode])


@pytest.mark.parametrize("name", sorted(bow_cases.FAMILY_CASES))
def test_search_family_cases(matcher, name):
    """both overloads x rotation check x nn_ratio 0.7 / 0.9, the eight settings of a case in one batched call"""
    a, b = bow_cases.family_pair(name)
    probs = [dict(a=a, b=b, mode=mode, nn_ratio=ratio, check_orientation=ori) for mode, ori, ratio in bow_cases.SETTINGS]
    res = matcher.SearchByBoWBatch(probs)
    for (mode, ori, ratio), (n, match) in zip(bow_cases.SETTINGS, res):
        rn, rmatch = bow_cases.family_reference(name, mode, ori, ratio)
        assert np.array_equal(match, rmatch), (name, mode, ori, ratio, np.argwhere(match != rmatch)[:5].ravel())
        assert n == rn, (name, mode, ori, ratio)


@pytest.mark.parametrize("name", ["empty_a", "empty_b", "both_empty", "disjoint", "no_nodes"])
def test_search_degenerate_cases(matcher, name):
    a, b = bow_cases.degenerate_pairs()[name]
    for mode in (0, 1):
        n, match = matcher.SearchByBoWBatch([dict(a=a, b=b, mode=mode, nn_ratio=0.9, check_orientation=1)])[0]
        assert n == 0 and len(match) == (len(b["node"]) if mode == 0 else len(a["node"])) and (match == -1).all()
        assert so.search_by_bow(a, b, mode, 0.9, 1)[0] == 0


def test_search_frame_side_needs_no_points_in_mode_0(matcher):
    a, b = bow_cases.family_pair("unequal")
    bare = {k: b[k] for k in ("desc", "angle", "node")}
    got = matcher.SearchByBoWBatch([dict(a=a, b=bare, mode=0, nn_ratio=0.7, check_orientation=1)])[0]
    rn, rmatch = bow_cases.family_reference("unequal", 0, 1, 0.7)
    assert got[0] == rn and np.array_equal(got[1], rmatch)


def test_search_mixed_batch_one_problem_beyond_the_limit(matcher):
    a, b = bow_cases.family_pair("nodes12")
    big = bow_cases.oversized_side()
    probs = [dict(a=a, b=b, mode=0, nn_ratio=0.9, check_orientation=1), dict(a=big, b=b, mode=1, nn_ratio=0.9, check_orientation=0),
             dict(a=a, b=b, mode=1, nn_ratio=0.7, check_orientation=0)]
    with pytest.raises(Exception) as e:
        matcher.SearchByBoWBatch(probs)
    assert e.value.code == -3
    res = matcher.SearchByBoWBatch(probs, partial_ok=True)
    assert res[1][0] == -1 and (res[1][1] == -3).all()             # untouched
    for got, key in ((res[0], (0, 1, 0.9)), (res[2], (1, 0, 0.7))):
        rn, rmatch = bow_cases.family_reference("nodes12", *key)
        assert got[0] == rn and np.array_equal(got[1], rmatch)


def test_search_vocabulary_and_matcher_on_one_device_only(matcher):
    """(a single-GPU box cannot build the cross-device pair; the check is that the same-device call is accepted)"""
    voc = _device_vocabulary("hand")
    assert voc.device == 0 and not voc.transform([bow_cases.HAND_FEATURES], 0, matcher=matcher)[0]["failed"]


# ---- chain: ComputeBoW on two views, SearchByBoW on the device's nodes, PoseOptimization (TrackReferenceKeyFrame) --------------
def test_chain_transform_search_pose(matcher):
    kf, cur = keyframes.bow_pair(31, na=300, nb=300, families=(40, 6, 8), flip_bits=4)
    name = "full_k10_L3"
    voc = _device_vocabulary(name)
    ta, tb = voc.transform([kf["desc"], cur["desc"]], 2, matcher=matcher)          # nodes at level 1: ten of them
    ref_voc = bow_cases.second_opinion_vocabulary(name)
    for t, side in ((ta, kf), (tb, cur)):
        _check_transform(t, ref_voc.transform(side["desc"], 2), len(side["desc"]), "chain")
    a = dict(kf, node=ta["node"], has_point=((kf["occupied"] != 0) & (kf["depth"] > 0)).astype(np.uint8))
    b = dict(cur, node=tb["node"])
    n, match = matcher.SearchByBoWBatch([dict(a=a, b=b, mode=0, nn_ratio=0.7, check_orientation=1)])[0]
    rn, rmatch = so.search_by_bow(a, b, 0, 0.7, 1)
    assert n == rn and np.array_equal(match, rmatch)
    assert n >= 15                                                                 # Tracking.cc:2941
    # the matched MapPoints: the keyframe's stereo points, in the world frame (the keyframe sits at the origin)
    fx, fy, cx, cy = [float(v) for v in kf["K8"][:4]]
    src = np.maximum(match, 0)
    z = kf["depth"][src].astype(np.float64)
    xw = np.stack([(kf["x"][src] - cx) * z / fx, (kf["y"][src] - cy) * z / fy, z], 1).astype(F32)
    sig2 = np.asarray(cur["level_sigma2"], F32)
    frame = dict(xw=xw, obs=np.stack([cur["x"], cur["y"], cur["u_right"]], 1).astype(F32), inv_sigma2=(F32(1) / sig2[cur["octave"]]).astype(F32),
                 valid=(match >= 0).astype(np.uint8), K=(fx, fy, cx, cy, float(kf["K8"][7])), tcw0=np.eye(4, dtype=F32))
    opt = Optimizer()
    inliers, tcw, outlier = opt.PoseOptimization([frame])[0]
    opt.close()
    assert inliers >= 10                                                           # Tracking.cc:2968
