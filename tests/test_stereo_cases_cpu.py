"""CPU checks on the randomised sweep of the stereo matcher (tests/stereo_cases.py), under the very seed and budget
tests/test_random_sweeps_gpu.py runs tools/stress_stereo.py with: the oracle and the second opinion agree bit for bit on every scene
(none is skipped), the scenes stay inside the documented input limits, and the run reaches every exit of the matching loop that keys
inside the image can reach - conditions on the inputs, checked on the reference."""
import math

import numpy as np
import pytest

import orb_second_opinion as so
import stereo_cases as sc
import sweep_cases

SEED, BUDGET = sweep_cases.COMMITTED["stereo"]


@pytest.fixture(scope="module")
def sweep():
    return sc.scenes(SEED, BUDGET), sc.references(SEED, BUDGET)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_oracle_and_second_opinion_agree_on_every_scene(sweep):
    scenes, refs = sweep
    assert len(scenes) == len(refs) == BUDGET
    compared = 0
    for i, (s, (orc, cnt)) in enumerate(zip(scenes, refs)):
        assert len(orc) == len(cnt) == len(s["pairs"])
        for p, ((kept, ur, dp), (kept2, ur2, dp2, c)) in enumerate(zip(orc, cnt)):
            assert len(ur) == len(dp) == len(ur2) == len(dp2) == c["n_left"], (i, p)
            assert kept == kept2, (i, p, kept, kept2)
            assert np.array_equal(_bits(ur), _bits(ur2)), (i, p, int((_bits(ur) != _bits(ur2)).sum()))
            assert np.array_equal(_bits(dp), _bits(dp2)), (i, p, int((_bits(dp) != _bits(dp2)).sum()))
            assert kept == int((dp > 0).sum()) == c["accepted"] - c["median_cut"], (i, p)
            compared += 1
    assert compared == sum(len(s["pairs"]) for s in scenes) >= BUDGET + 9


def test_scenes_are_inside_the_input_limits(sweep):
    scenes, _ = sweep
    n_img = BUDGET // 2
    assert [s["kind"] for s in scenes] == ["image"] * n_img + ["keys"] * (BUDGET - n_img) and n_img >= 12 and BUDGET - n_img >= 12
    for s in scenes:
        assert s["levels"] in sc.LEVELS and s["scale"] in sc.SCALES and s["nfeatures"] in sc.NFEATURES
        assert s["levels"] <= 4 or s["scale"] != 2.0
        side = int(math.ceil(70 * s["scale"] ** (s["levels"] - 1))) + 8
        assert side <= s["h"] <= s["w"] <= 640, (s["w"], s["h"], side)
        assert s["mb"] > 0 and s["mbf"] > 0
        for left, right in s["pairs"]:
            assert left.shape == right.shape == (s["h"], s["w"]) and left.dtype == right.dtype == np.uint8
    # the batch: ten pairs of one size, the blank pair in the middle, pairs 8 and 9 not blank
    kinds = scenes[0]["pair_kinds"]
    assert len(kinds) >= 10 and kinds[8] == kinds[9] == "stereo" and "blank" in kinds[3:7] and "right_blank" in kinds and "same" in kinds
    assert all(len(s["pairs"]) == 1 for s in scenes[1:])
    every = [k for s in scenes for k in s["pair_kinds"]]
    assert {"stereo", "same", "blank", "right_blank"} <= set(every)
    # maxD = mbf / mb: below one pixel, a few pixels, the scene's disparities, beyond the image width (minU < 0 for every key)
    for kind_of in ("image", "keys"):
        max_d = [(np.float32(s["mbf"]) / np.float32(s["mb"]), s) for s in scenes if s["kind"] == kind_of]
        assert any(d < 1 for d, _ in max_d) and any(2 <= d <= 6 for d, _ in max_d) and any(d > s["w"] for d, s in max_d)
        assert any(s["bf"] / 6 < d < s["w"] for d, s in max_d)


def test_key_sets_are_what_the_issue_asks_for(sweep):
    scenes, _ = sweep
    keys = [s for s in scenes if s["kind"] == "keys"]
    assert {len(s["kps_l"]) for s in keys} == set(sc.N_LEFT) and {len(s["kps_r"]) for s in keys} == set(sc.N_RIGHT)
    assert sum(len(s["kps_r"]) < 10 for s in keys) >= 3
    assert {"stereo", "same"} == {s["pair_kinds"][0] for s in keys}
    pop = np.array([bin(i).count("1") for i in range(256)], np.int64)
    seen_flips, seen_shift = set(), set()
    for s in keys:
        w, h = s["w"], s["h"]
        for k in (s["kps_l"], s["kps_r"]):
            assert ((k["x"] >= 0) & (k["x"] < w) & (k["y"] >= 0) & (k["y"] < h)).all()
            assert ((k["octave"] >= 0) & (k["octave"] < s["levels"])).all()
        assert s["desc_l"].shape == (len(s["kps_l"]), 32) and s["desc_r"].shape == (len(s["kps_r"]), 32)
        src, flips = s["made"]["src"], s["made"]["flips"]
        assert np.array_equal(pop[s["desc_r"] ^ s["desc_l"][src]].sum(axis=1), flips)                  # exactly k bits
        seen_flips |= set(flips.tolist())
        seen_shift |= set((s["kps_r"]["octave"] - s["kps_l"]["octave"][src]).tolist())
        if len(src) >= 300:
            assert not np.array_equal(src, np.sort(src))                                               # shuffled
    assert seen_flips == set(sc.FLIPS) and seen_shift == {-2, -1, 0, 1, 2}
    big = max(keys, key=lambda s: len(s["kps_l"]))
    k, w, h = big["kps_l"], big["w"], big["h"]
    assert len(k) == 4096 and set(k["octave"].tolist()) == set(range(big["levels"])) and big["levels"] >= 3
    share = lambda m: float(np.mean(m))
    assert share(k["x"] < 12) > 0.1 and share(k["x"] >= w - 14) > 0.1 and share((k["y"] < 6) | (k["y"] >= h - 6)) > 0.1
    assert share(np.isin(k["y"].astype(np.int64) % 8, (1, 7))) > 0.3
    assert 0.3 < share((k["x"] == np.floor(k["x"])) & (k["y"] == np.floor(k["y"]))) < 0.5
    # rows moved to the edge of the band and 1.01 past it
    kr, src = big["kps_r"], big["made"]["src"]
    dy = np.abs(kr["y"].astype(np.float64) - k["y"][src])
    band = 2.0 * so.scale_tables(big["levels"], big["scale"])[0][kr["octave"]].astype(np.float64)
    assert share(dy == 0) > 0.4 and share(np.abs(dy - band) < 1e-4) > 0.1 and share(np.abs(dy - band - 1.01) < 1e-4) > 0.1


def _totals(refs):
    tot = {g: 0 for g in sc.GATES}
    for _, cnt in refs:
        for _, _, _, c in cnt:
            for g in sc.GATES:
                tot[g] += c[g]
    return tot


def test_the_run_reaches_every_gate(sweep):
    scenes, refs = sweep
    tot = _totals(refs)
    for gate in ("hamming", "endu", "sad_edge", "negative", "beyond_max_d", "median_cut", "empty_row", "tie", "win_74", "loss_75"):
        assert tot[gate] >= 20, (gate, tot)
    assert tot["zero_clamp"] >= 10, tot
    per_pair = [(s, c) for s, (_, cnt) in zip(scenes, refs) for _, _, _, c in cnt]
    accepted = [c["accepted"] for _, c in per_pair]
    assert 1 in accepted and 2 in accepted and max(accepted) > 1000
    assert any(c["accepted"] > 0 and c.get("median") == 0 for _, c in per_pair)                            # median SAD 0: nothing survives the cut
    assert any(c["n_right"] == 0 and c["n_left"] > 0 for s, c in per_pair if s["kind"] == "image")     # Nr == 0 with N > 0 ...
    assert any(c["n_right"] == 0 and c["n_left"] > 0 for s, c in per_pair if s["kind"] == "keys")      # ... on both entries
    assert any(c["n_left"] == 0 for _, c in per_pair)                                                  # the blank pair
    for kind_of in ("image", "keys"):
        assert {s["levels"] for s in scenes if s["kind"] == kind_of} == set(sc.LEVELS)
        assert {s["scale"] for s in scenes if s["kind"] == kind_of} == set(sc.SCALES)
    # the exits that keys inside the image cannot take (the module's docstring says why) stay untaken
    assert not any(c.get(g) for _, c in per_pair for g in ("max_u_negative", "iniu", "delta", "nan_parabola"))
    # pairs 8 and 9 of the batch - the second grid row of st_match - have matches to get wrong
    assert all(c["accepted"] > 50 for _, c in per_pair[8:10])


def test_the_docstring_holds_the_counts_of_the_committed_run(sweep):
    _, refs = sweep
    assert sc.counts_line(_totals(refs)) in " ".join(sc.__doc__.split())


def test_border_argument_reads_the_same_pixels(sweep):
    """stereo_matches on the padded planes at an offset gives what it gives on the unpadded levels wherever the latter is defined (the
    extractor's keypoints keep 19 pixels from the border of their level)"""
    scenes, refs = sweep
    i = next(i for i, s in enumerate(scenes) if s["kind"] == "image" and s["pair_kinds"] == ("stereo",) and refs[i][1][0][3]["accepted"] > 100)
    s = scenes[i]
    ol, orr, kl, dl, kr, dr = sc.extracted(s, 0)
    sf, isf = so.scale_tables(s["levels"], s["scale"])
    e = so.EDGE
    plain = [[x.padded(l)[e:-e, e:-e] for l in range(s["levels"])] for x in (ol, orr)]
    counts = {}
    got = so.stereo_matches(kl, dl, kr, dr, plain[0], plain[1], sf, isf, np.float32(s["mb"]), np.float32(s["mbf"]), counts=counts)
    kept, ur, dp, c = refs[i][1][0]
    assert got[0] == kept and np.array_equal(_bits(got[1]), _bits(ur)) and np.array_equal(_bits(got[2]), _bits(dp))
    assert all(counts.get(g, 0) == c[g] for g in sc.GATES)
