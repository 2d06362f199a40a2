"""CPU checks on the parity sweep of the tracking thread's matchers (tests/match_cases.py), under the very seed and budget
tests/test_random_sweeps_gpu.py runs tools/stress_matchers.py --cases with: the compiled oracle and the counted second opinion agree
bit for bit on every problem of every scene (none is skipped), the scenes stay inside the documented input limits and their shapes are
the issue's lists, the hand-built facts hold, and the run reaches every gate of the searches - conditions on the inputs, checked on
the reference alone."""
import numpy as np
import pytest

import match_cases as mc
import match_second_opinion as ms
import sweep_cases

SEED, BUDGET = sweep_cases.COMMITTED["match"]
F32 = np.float32
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


@pytest.fixture(scope="module")
def sweep():
    return mc.scenes(SEED, BUDGET), mc.references(SEED, BUDGET)


@pytest.fixture(scope="module")
def totals(sweep):
    return mc.totals_of(sweep[1])


def _family(scenes, kind, family=None):
    return [s for s in scenes if s["kind"] == kind and (family is None or s["family"] == family)]


def test_oracle_and_second_opinion_agree_on_every_problem(sweep):
    scenes, refs = sweep
    assert len(scenes) == len(refs) == BUDGET
    compared = 0
    for i, (s, ref) in enumerate(zip(scenes, refs)):
        assert len(ref) == len(s["problems"])
        for p, r in enumerate(ref):
            for check_ori in (True, False):
                a, b = r["oracle"][check_ori], r["second"][check_ori]
                where = (i, s["kind"], s["family"], p, r["mode"], check_ori)
                if r["mode"] == "fuse":
                    assert a[0].dtype == b[0].dtype == a[1].dtype == b[1].dtype == np.int32
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), where + (int((a[0] != b[0]).sum()), int((a[1] != b[1]).sum()))
                else:
                    assert a[0] == b[0], where + (a[0], b[0])
                    assert a[1].dtype == b[1].dtype == np.int32 and np.array_equal(a[1], b[1]), where + (int((a[1] != b[1]).sum()),)
                    kept = int((a[1] >= 0).sum())
                    assert a[0] >= kept and (a[0] == kept or r["mode"] != "bf")          # (an overwritten keypoint counts twice, as in the reference)
                compared += 1
    # 26 projection scenes of 3 problems (one of 65), 9 brute-force scenes, 4 Fuse scenes of 3; both settings of check_ori
    assert compared == 2 * sum(len(s["problems"]) for s in scenes) == 2 * 245


def test_scenes_are_inside_the_input_limits_and_have_the_stated_shapes(sweep, totals):
    scenes, refs = sweep
    general = _family(scenes, "proj", "general") + _family(scenes, "proj", "hist")
    assert {len(s["problems"][0]["train"]["x"]) for s in general} == set(mc.P_TRAIN)
    assert {len(s["problems"][0]["query"]["valid"]) for s in general} == set(mc.P_QUERY)
    assert [len(s["problems"][0]["train"]["x"]) for s in _family(scenes, "proj", "collide")] == list(mc.COLLIDE_TRAIN)
    bf = [p for s in _family(scenes, "bf") for p in s["problems"]]
    assert {len(p["t_desc"]) for p in bf} == set(mc.BF_NT) and {len(p["q_desc"]) for p in bf} == set(mc.BF_NQ)
    assert all(len(p["q_desc"]) <= 63 for p in bf if len(p["t_desc"]) == 4096)                       # only the smallest query sets with the largest train set
    assert max(len(p["t_desc"]) for p in bf) == 4096                                                 # PS_BF_MAX_TRAIN
    fuse = [p for s in _family(scenes, "fuse") for p in s["problems"]]
    assert {len(p["train"]["x"]) for p in fuse} <= set(mc.P_TRAIN) and {len(p["query"]["valid"]) for p in fuse} <= set(mc.P_QUERY)
    assert {1, 63, 64, 65, 1000} <= {len(p["train"]["x"]) for p in fuse} and {0, 1, 63, 64, 65, 600} <= {len(p["query"]["valid"]) for p in fuse}
    for s in scenes:
        for pr in s["problems"]:
            if s["kind"] == "bf":
                continue
            T = pr["train"]
            assert len(T["x"]) <= 32767
            # Grid.__init__ (C round on the float32 product) and build_grid put every keypoint into the same cell or outside
            g = ms.Grid(T["x"], T["y"], T["grid"])
            off, idx = T["cell_off"], T["cell_idx"]
            cells = [list(idx[off[c]:off[c + 1]]) for c in range(64 * 48)]
            assert cells == [g.cells[c // 48][c % 48] for c in range(64 * 48)]
    # no window beyond the wide key format's 1024 candidates; the wide scene's train set fits its 13 index bits
    assert not any(totals[m].get("over_1024_candidates") for m in mc.MODES)
    (wide,) = _family(scenes, "proj", "wide")
    dense = wide["problems"][1]
    assert len(wide["problems"]) == 3 and dense["mode"] == "points" and 600 <= len(dense["train"]["x"]) <= 1000
    # images 200 x 120 .. 640 x 376; two grids and more with their origin off zero, on either side, keypoints on the bounds and outside the grid
    made = [m for s in _family(scenes, "proj") for m in s["made"]]
    assert all(200 <= m["size"][0] <= 640 and 120 <= m["size"][1] <= 376 for m in made)
    for origin, sign in (("negative", -1), ("positive", 1)):
        off_zero = [s for s in _family(scenes, "proj", "general") if s["made"][0]["origin"] == origin]
        assert len(off_zero) >= 2
        for s in off_zero:
            T, b = s["problems"][0]["train"], s["problems"][0]["bounds"]
            assert sign * T["grid"][0] > 0 and sign * T["grid"][1] > 0 and b[0] == T["grid"][0] and b[2] == T["grid"][1]
            if len(T["x"]) >= 300:
                assert len(T["cell_idx"]) < len(T["x"])                                              # some keypoints are in no cell
                assert ((T["x"] == b[0]) | (T["x"] == b[1]) | (T["y"] == b[2]) | (T["y"] == b[3])).any()
    # each motion branch at least twice, on different scenes
    for motion in mc.MOTIONS:
        assert sum(r["counts"].get(motion, 0) > 0 for s, ref in zip(scenes, refs) if s["family"] != "batch" for r in ref) >= 2, motion
    # the batch: 65 problems of at most 64 trains and 70 queries, ten of them empty on either side, all three modes
    (batch,) = _family(scenes, "proj", "batch")
    sizes = [(len(p["train"]["x"]), len(p["query"]["valid"])) for p in batch["problems"]]
    assert len(sizes) == 65 and max(n for n, _ in sizes) <= 64 and max(m for _, m in sizes) <= 70
    assert sum(n == 0 for n, _ in sizes) == 5 and sum(m == 0 for _, m in sizes) == 5
    assert {mc.mode_of(batch, p) for p in batch["problems"]} == {"frame", "points", "object"}


def test_hand_built_facts_hold(sweep):
    scenes, refs = sweep
    seen_flips, seen_bf_flips, n_collisions, n_bf_collisions, n_pairs = set(), set(), 0, 0, 0
    for s, ref in zip(scenes, refs):
        if s["kind"] == "proj" and s["family"] != "batch":
            made, pr = s["made"][0], s["problems"][0]
            T, q = pr["train"], pr["query"]
            for row, i, k in made["flips"]:                                                          # exactly k bits
                assert int(_POP[T["desc"][row] ^ q["desc"][i]].sum()) == k
                seen_flips.add(k)
            points = next(r for r, p in zip(ref, s["problems"]) if r["mode"] == "points" and p["train"] is T)
            for qa, qb, ta, tb in made["collisions"]:
                # equal modulo the claim table's size, the earlier lane first in one 64-query block - and each query does get its train
                assert (tb - ta) % 4096 == 0 and ta != tb and qa < qb and qa // 64 == qb // 64
                assert points["second"][True][1][ta] == qa and points["second"][True][1][tb] == qb
                n_collisions += 1
            for i, best, second, other, r1, r2 in made["ratio"]:
                assert int(_POP[T["desc"][r1] ^ q["desc"][i]].sum()) == best and int(_POP[T["desc"][r2] ^ q["desc"][i]].sum()) == second
                assert (T["octave"][r1] != T["octave"][r2]) == other
                n_pairs += 1
        if s["kind"] == "bf":
            for made, p, r in zip(s["made"], s["problems"], ref):
                for row, i, k in made["flips"]:
                    assert int(_POP[p["t_desc"][row] ^ p["q_desc"][i]].sum()) == k
                    seen_bf_flips.add(k)
                for qa, qb, ta, tb in made["collisions"]:
                    assert (tb - ta) % 512 == 0 and ta != tb and qb == qa + 1 and qa // 64 == qb // 64
                    assert not (p["q_desc"][qa] ^ p["t_desc"][ta]).any() and not (p["q_desc"][qb] ^ p["t_desc"][tb]).any()
                    assert r["second"][False][1][ta] == qa and r["second"][False][1][tb] == qb
                    n_bf_collisions += 1
        if s["kind"] == "fuse":
            for made, p in zip(s["made"], s["problems"]):
                for row, i, k in made["flips"]:
                    assert int(_POP[p["train"]["desc"][row] ^ p["query"]["desc"][i]].sum()) == k
                if made["extra"] >= 100:                                                             # a cell with more than 64 features
                    assert np.diff(p["train"]["cell_off"]).max() > 64
    assert seen_flips >= set(mc.P_FLIPS) | set(mc.BLOCK_DISTANCES) and seen_bf_flips >= set(mc.BF_FLIPS)
    assert n_collisions >= 10 and n_bf_collisions >= 10 and n_pairs >= 100
    # the ratio pairs lie on the float boundary: the rejection `best > nnratio * second` and the acceptance `best < nnratio * second` both fail on them
    for nnratio, pairs in mc.RATIO_PAIRS.items():
        assert len(pairs) >= 4
        for best, second in pairs:
            assert F32(best) == F32(nnratio) * F32(second), (nnratio, best, second)
    # each step of a ladder passes its ratio test against the next (brute force: as far as TH_LOW lets a step be accepted at all)
    for ladder_ratio, ladder in list(mc.BF_LADDER.items()) + [(r, mc.BLOCK_DISTANCES) for r in mc.RATIO_PAIRS]:
        limit = 100 if ladder is mc.BLOCK_DISTANCES else 50
        assert all(F32(a) < F32(ladder_ratio) * F32(b) for a, b in zip(ladder, ladder[1:]) if a <= limit)
        assert sum(a <= limit for a in ladder) >= (6 if ladder is mc.BLOCK_DISTANCES else 8)
    # blocks of 5 to 70 consecutive queries on one to six trains, some across two 64-query blocks, observed and unobserved queries inside
    blocks = [(b, s["problems"][0]["query"]["observed"]) for s in _family(scenes, "proj", "general") for b in s["made"][0]["blocks"]]
    assert {5, 70} <= {b[1] for b, _ in blocks} and {1, 6} <= {b[2] for b, _ in blocks}
    assert any(b[0] // 64 != (b[0] + b[1] - 1) // 64 for b, _ in blocks)
    assert all(0 < obs[b[0]:b[0] + b[1]].sum() < b[1] for b, obs in blocks if b[1] >= 9)


# (mode, gate, lower bound): 20 for the ordinary gates, 10 for the exact boundaries and the fall-back paths, 2 for the rare shapes
_ORDINARY = {
    "frame": ("invalid", "behind_camera", "out_of_bounds", "empty_window", "all_filtered", "level_skip", "ur_gate", "blocked_at_entry", "blocked_by_call",
              "over_limit", "accepted", "bin_wrap_30", "removed_by_rotation", "window_over_16_columns"),
    "points": ("invalid", "empty_window", "all_filtered", "level_skip", "ur_gate", "blocked_at_entry", "blocked_by_call", "over_limit", "ratio_reject",
               "ratio_saved_by_level", "single_candidate", "accepted", "window_over_16_columns"),
    "object": ("invalid", "empty_window", "all_filtered", "level_skip", "bbox_skip", "ur_gate", "blocked_at_entry", "blocked_by_call", "over_limit", "ratio_reject",
               "ratio_saved_by_level", "single_candidate", "accepted"),
    "bf": ("invalid", "blocked_by_call", "over_limit", "ratio_reject", "single_candidate", "accepted", "accepted_not_first_choice", "bin_wrap_30", "removed_by_rotation"),
    "fuse": ("invalid", "behind_camera", "outside_bounds", "outside_distance_range", "view_angle", "level_clamped_low", "level_clamped_high", "level_skip",
             "chi2_stereo", "chi2_mono", "tie_at_best", "best_eq_50", "best_eq_51", "accepted"),
}
_EXACT = {
    "frame": ("best_eq_limit", "best_eq_limit_plus_1", "scan_path", "tie_at_best", "overwrite_unobserved"),
    "points": ("best_eq_limit", "best_eq_limit_plus_1", "ratio_equality_same_level", "ratio_equality_other_level", "scan_path", "tie_at_best", "overwrite_unobserved"),
    "object": ("best_eq_limit", "best_eq_limit_plus_1", "ratio_equality_same_level", "ratio_equality_other_level", "scan_path", "tie_at_best", "overwrite_unobserved"),
    "bf": ("best_eq_limit", "best_eq_limit_plus_1", "ratio_equality", "rescan", "tie_at_best"),
}
_RARE = {"frame": ("hist_kept_1", "hist_kept_2", "hist_kept_3", "hist_on_tenth_boundary", "hist_equal_bins", "forward", "backward", "neither", "mono"),
         "points": ("over_256_candidates",), "bf": ("hist_kept_1", "hist_kept_2", "hist_kept_3", "hist_on_tenth_boundary", "hist_equal_bins", "no_train_left")}


def test_the_run_reaches_every_gate(totals):
    for bound, table in ((20, _ORDINARY), (10, _EXACT), (2, _RARE)):
        for mode, gates in table.items():
            for gate in gates:
                assert totals[mode].get(gate, 0) >= bound, (mode, gate, totals[mode].get(gate, 0), bound)


def test_the_histograms_are_the_planned_ones(sweep):
    """the scenes planned bin by bin end as planned: the frame problems and the brute-force problems keep 1, 2 and 3 maxima, sit on
    the 0.1f * max1 boundary with 10 and 1 and with 20 and 2 matches, and one match below it loses its bin"""
    scenes, refs = sweep
    for kind, mode in (("proj", "frame"), ("bf", "bf")):
        seen = {}
        for s, ref in zip(_family(scenes, kind, "hist"), [r for s, r in zip(scenes, refs) if s["kind"] == kind and s["family"] == "hist"]):
            for made, r in zip(s["made"] if kind == "bf" else s["made"] * 3, ref):
                if r["mode"] == mode:
                    c = r["counts"]
                    seen[made["plan"]] = (c.get("accepted", 0), [k for k in (1, 2, 3) if c.get("hist_kept_%d" % k)], c.get("hist_on_tenth_boundary", 0), c.get("removed_by_rotation", 0))
        assert set(seen) == set(mc.HIST_PLANS)
        for plan, (accepted, kept, boundary, removed) in seen.items():
            assert accepted == sum(plan), (mode, plan, accepted)
        assert seen[(11, 1)][1:] == ([1], 0, 1) and seen[(10, 1)][1:] == ([2], 1, 0) and seen[(20, 2)][1:] == ([2], 1, 0)
        assert seen[(10, 10)][1:] == ([2], 0, 0) and seen[(10, 5, 3)][1:] == ([3], 0, 0) and seen[(10, 5, 1)][1:] == ([3], 1, 0)
        assert seen[(12,)][1:] == ([1], 0, 0) and seen[(10, 1, 1)][1:] == ([3], 1, 0)


def test_the_docstring_holds_the_counts_of_the_committed_run(totals):
    assert " ".join(mc.counts_line(totals).split()) in " ".join(mc.__doc__.split())


def test_counting_does_not_alter_results(sweep):
    """the counted call is the call compared: with and without a counts dict the second opinion answers the same"""
    scenes, refs = sweep
    for s, ref in list(zip(scenes, refs))[:8]:
        for pr, r in zip(s["problems"], ref):
            plain = mc.second_opinion(s, pr, True)
            assert np.array_equal(plain[0], r["second"][True][0]) and np.array_equal(plain[1], r["second"][True][1])
