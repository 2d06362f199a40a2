"""The scenes of the parity sweep over the tracking thread's matchers (tools/stress_matchers.py --cases: SearchByProjection in its
frame, local-map and object modes, SearchByBruceMatching, FuseSearch) and of tests/test_match_cases_cpu.py.  scenes(seed, budget) is a
deterministic list of calls - dict(kind = "proj" / "bf" / "fuse", nnratio, problems = the problems of ONE call, made = the hand-built
facts) - drawn through sweep_cases._Draw on pointslot_amd.synth's generator; pure numpy, no GPU code.  Test infrastructure.

Input limits every scene stays inside: a brute-force problem has at most PS_BF_MAX_TRAIN = 4096 train descriptors, a searched frame
at most 32 767 features (8191 where a window holds more than 256 candidates), a search window at most 1024 candidates.

Projection scenes (frame + local-map + object problem on one searched side): train and query counts from P_TRAIN x P_QUERY, images
200 x 120 .. 640 x 376, grids whose origin is negative or positive with keypoints on the bounds and outside the grid, the four
motion branches of the frame mode, points behind the camera and around every bound, train keys built around each query (copies of its
descriptor with exactly k flipped bits, groups at one distance, (best, second) pairs on the float ratio boundary and one off it at
the same and at another octave, u_right `radius` from the projected uR, octaves level - 2 .. level + 2), blocks of consecutive queries
that want the same one to six trains, rotations that wrap from bin 30 to 0 and sit on x.5 bin boundaries, histograms planned bin by
bin.  Beside them two scenes with 4097 and more trains where a query's train equals an earlier lane's modulo 4096, one scene with a
300-to-700-candidate window (the wide key format) and one call of 65 small problems.  Brute-force scenes: BF_NT x BF_NQ, trains at k
flipped bits of their query, groups of queries sharing one best train among near-duplicates (the eight-key lists run out), more
queries than trains, train indices equal modulo 512 wanted by neighbouring lanes.  Fuse scenes: synth.fuse_scene plus candidates and
features placed on each gate's boundary (bounds taken from the projections themselves) and a cell with more than 64 features.

The counted second opinion (tests/match_second_opinion.py, counts=) passes the gates as follows under the committed seed and budget,
sweep_cases.COMMITTED["match"] (tests/test_match_cases_cpu.py asserts the issue's lower bounds on them):

    frame: accepted 1576, all_filtered 963, backward 12, behind_camera 84, best_eq_limit 58, best_eq_limit_plus_1 38, bin_wrap_30
        138, blocked_at_entry 434, blocked_by_call 7308, empty_window 697, forward 14, hist_equal_bins 11, hist_kept_1 10,
        hist_kept_2 14, hist_kept_3 17, hist_on_tenth_boundary 4, invalid 665, level_skip 12268, mono 11, neither 10, out_of_bounds
        256, over_limit 806, overwrite_unobserved 101, removed_by_rotation 526, scan_path 1097, tie_at_best 256, ur_gate 1366,
        window_over_16_columns 40
    points: accepted 1356, all_filtered 741, best_eq_limit 57, best_eq_limit_plus_1 34, blocked_at_entry 982, blocked_by_call 7126,
        empty_window 1040, invalid 669, level_skip 18652, over_256_candidates 40, over_limit 889, overwrite_unobserved 84,
        ratio_equality_other_level 92, ratio_equality_same_level 172, ratio_reject 256, ratio_saved_by_level 52, scan_path 1062,
        single_candidate 401, tie_at_best 225, ur_gate 857, window_over_16_columns 66
    object: accepted 1592, all_filtered 1082, bbox_skip 524, best_eq_limit 39, best_eq_limit_plus_1 26, blocked_at_entry 161,
        blocked_by_call 6456, empty_window 1057, invalid 680, level_skip 3033, over_limit 205, overwrite_unobserved 90,
        ratio_equality_other_level 69, ratio_equality_same_level 145, ratio_reject 315, ratio_saved_by_level 104, scan_path 1027,
        single_candidate 689, tie_at_best 193, ur_gate 110
    bf: accepted 1567, accepted_not_first_choice 634, best_eq_limit 110, best_eq_limit_plus_1 92, bin_wrap_30 93, blocked_by_call
        2665, hist_equal_bins 32, hist_kept_1 32, hist_kept_2 9, hist_kept_3 35, hist_on_tenth_boundary 4, invalid 996,
        no_train_left 1169, over_limit 4668, ratio_equality 293, ratio_reject 568, removed_by_rotation 701, rescan 512,
        single_candidate 24, tie_at_best 777
    fuse: accepted 615, behind_camera 81, best_eq_50 41, best_eq_51 44, chi2_mono 271, chi2_stereo 664, empty_window 2, invalid 94,
        level_clamped_high 176, level_clamped_low 34, level_skip 4277, outside_bounds 194, outside_distance_range 55, tie_at_best
        48, view_angle 104

(best_eq_limit / best_eq_limit_plus_1: the best distance is exactly the mode's threshold - 100, 130 for the object mode, 50 for the brute
force - or one beyond it; scan_path: more than four candidates free at entry and fewer of the four best still unclaimed than the
decision reads, where the device walks the whole candidate list; rescan: fewer than two of a brute-force query's eight smallest keys
still untaken; ratio_equality*: float(best) == nnratio * float(second) exactly; ratio_saved_by_level: the ratio test would reject, the
two octaves differ; hist_on_tenth_boundary: max2 or max3 equal to 0.1f * max1; window_over_16_columns: the device walks a window 16
grid columns at a time.)  tools/stress_matchers.py 20250503 - the 60 random scenes that were the only sweep of these matchers before -
passes them as follows (random_run_totals(), some 20 s of pure Python; not part of the suite):

    frame: accepted 17663, all_filtered 16746, best_eq_limit 17, best_eq_limit_plus_1 33, bin_wrap_30 96, blocked_at_entry 23587,
        blocked_by_call 133571, empty_window 8496, forward 60, hist_equal_bins 25, hist_kept_1 54, hist_kept_2 3, hist_kept_3 3,
        hist_on_tenth_boundary 3, invalid 6695, level_skip 966073, over_limit 16320, overwrite_unobserved 835, removed_by_rotation
        2598, scan_path 713, tie_at_best 1008, ur_gate 84347, window_over_16_columns 985
    points: accepted 18711, all_filtered 19137, best_eq_limit 3, best_eq_limit_plus_1 18, blocked_at_entry 8060, blocked_by_call
        54029, empty_window 10171, invalid 6695, level_skip 495749, over_limit 11204, overwrite_unobserved 974, ratio_reject 2,
        ratio_saved_by_level 1, scan_path 966, single_candidate 10735, tie_at_best 355, ur_gate 26092
    object: accepted 23398, all_filtered 32083, bbox_skip 8695, best_eq_limit 309, best_eq_limit_plus_1 286, blocked_at_entry 3727,
        blocked_by_call 35974, empty_window 1133, invalid 6695, level_skip 45126, over_limit 2079, overwrite_unobserved 1534,
        ratio_equality_other_level 1, ratio_equality_same_level 1, ratio_reject 532, ratio_saved_by_level 805, scan_path 139,
        single_candidate 18173, tie_at_best 65, ur_gate 2568
    bf: accepted 4547, bin_wrap_30 19, blocked_by_call 4340, hist_equal_bins 18, hist_kept_1 28, hist_kept_2 14, hist_kept_3 18,
        invalid 2105, over_limit 13629, ratio_equality 4, ratio_reject 99, removed_by_rotation 903, rescan 34, tie_at_best 1809
    fuse: accepted 31364, behind_camera 1394, chi2_mono 1309, chi2_stereo 7317, empty_window 35, invalid 3691, level_skip 36031,
        outside_bounds 1900, outside_distance_range 1892, tie_at_best 4, view_angle 3446
"""
import functools
import math

import numpy as np

import match_second_opinion as ms
import oracle_lib
import sweep_cases
from pointslot_amd import synth
from pointslot_amd.matcher import build_grid
from stereo_cases import _flipped

F32 = np.float32
P_TRAIN = (1, 15, 16, 17, 63, 64, 65, 300, 1000)
P_QUERY = (0, 1, 3, 4, 5, 63, 64, 65, 129, 600)
COLLIDE_TRAIN = (4097, 4600)
BF_NT = (0, 1, 2, 7, 8, 9, 255, 256, 257, 511, 512, 513, 1024, 1025, 4096)
BF_NQ = (0, 1, 63, 64, 65, 130, 1000)
MOTIONS = ("forward", "backward", "neither", "mono")
P_FLIPS = (0, 10, 40, 49, 50, 51, 99, 100, 101, 129, 130, 131)
BF_FLIPS = (0, 18, 44, 45, 49, 50, 51)
RATIO_PAIRS = {0.6: ((3, 5), (6, 10), (12, 20), (18, 30), (24, 40)), 0.8: ((4, 5), (8, 10), (16, 20), (32, 40)),
               0.9: ((9, 10), (18, 20), (27, 30), (36, 40), (45, 50))}
# a block's trains lie at these distances from its queries: each passes every ratio test against the next
BLOCK_DISTANCES = (2, 8, 16, 30, 55, 95)
# ... and so do the near-duplicates of a brute-force group, up to TH_LOW
BF_LADDER = {0.6: (0, 1, 2, 4, 7, 12, 21, 36, 61, 70, 80, 90), 0.8: (0, 1, 2, 3, 4, 6, 8, 11, 14, 18, 23, 29, 37, 47, 60, 80),
             0.9: (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 21, 24, 27, 31, 35, 39, 44, 50)}
# histograms bin by bin (matches per bin, largest first): kept maxima 1 / 2 / 3, max2 on 0.1f * max1 (10 and 1, 20 and 2), one below, equal bins
HIST_PLANS = ((11, 1), (10, 1), (20, 2), (10, 10), (10, 5, 3), (10, 5, 1), (12,), (10, 1, 1))
_P_SIZES = ((1000, 600), (300, 129), (65, 65), (64, 64), (63, 63), (17, 5), (16, 4), (15, 3), (1, 1), (300, 0), (1000, 600), (1000, 600),
            (300, 129), (65, 600))
_P_ORIGIN = {4: "negative", 6: "positive", 10: "negative", 11: "positive"}
_HIST_SIZES = ((64, 65), (63, 64), (65, 63), (300, 64), (64, 129), (65, 65), (63, 63), (64, 64))
_BF_SHAPES = (((63, 2), (64, 7), (65, 8), (1, 1)), ((130, 9), (63, 0), (0, 256), (130, 255)), ((1000, 256), (130, 257)), ((1000, 511), (130, 512)),
              ((1000, 513), (130, 1024)), ((1000, 1025), (63, 4096), (1, 4096)), ((64, 1), (65, 2), (63, 7), (130, 8)))
_F_SIZES = ((1000, 600), (300, 129), (65, 65), (64, 64), (63, 63), (17, 5), (16, 4), (15, 3), (1, 1), (300, 0), (1000, 129), (300, 600))
MODES = ("frame", "points", "object", "bf", "fuse")


def _levels():
    s = [F32(1.0)]
    for _ in range(7):
        s.append(F32(np.float64(s[-1]) * np.float64(F32(1.2))))
    s = np.array(s, F32)
    return s, (F32(1.0) / (s * s)).astype(F32)


SF, INV_SIGMA2 = _levels()


def _rotations(rng, n):
    """query angle - train angle: most around 12 degrees, some in [354, 360) (bin 30 wraps to 0), some exactly on x.5 bin boundaries"""
    u = rng.uniform(n)
    half = 12.0 * (rng.integers(n, 0, 29) + 0.5)
    return np.where(u < 0.6, 12.0 + 2.0 * rng.normal(n), np.where(u < 0.72, 354.0 + 6.0 * rng.uniform(n) * 0.999, np.where(u < 0.85, half, 360.0 * rng.uniform(n))))


def _angle_pair(rng, rot):
    """(query angle, train angle) float32 with query - train == rot exactly: whole degrees and halves"""
    ta = np.floor(rng.uniform(len(rot)) * 300.0)
    return ((ta + rot) % 360.0).astype(F32), ta.astype(F32)


# ---- projection scenes -------------------------------------------------------------------------------------------------------------
def _camera(d, w, h, origin):
    off = dict(zero=(0.0, 0.0), negative=(-(d.int(3, 20) + 0.5), -(d.int(2, 12) + 0.25)), positive=(d.int(3, 20) + 0.5, d.int(2, 12) + 0.25))[origin]
    min_x, min_y = F32(off[0]), F32(off[1])
    max_x, max_y = F32(min_x + F32(w)), F32(min_y + F32(h))
    fx = F32(0.58 * w)
    K6 = (fx, fx, F32(min_x + F32(w) / 2), F32(min_y + F32(h) / 2), F32(0.54) * fx, F32(0.54))
    return (min_x, max_x, min_y, max_y), (min_x, min_y, F32(64) / F32(max_x - min_x), F32(48) / F32(max_y - min_y)), K6


def _poses(rng, motion, mb):
    tz = dict(forward=-(mb + 0.3), backward=mb + 0.3, neither=0.1, mono=-(mb + 0.3))[motion]
    tcw, tlw = np.eye(4, dtype=F32), np.eye(4, dtype=F32)
    tcw[:3, :3] = synth._so3_exp(np.radians(rng.uniform(3, -1.0, 1.0))); tcw[:3, 3] = np.array([0.05, -0.02, tz]) + rng.uniform(3, -0.03, 0.03)
    tlw[:3, :3] = synth._so3_exp(np.radians(rng.uniform(3, -0.3, 0.3))); tlw[:3, 3] = rng.uniform(3, -0.02, 0.02)
    return tcw, tlw


class _Trains:
    """the searched side while it is being built: rows are appended, `made` remembers what each hand-built row is"""

    def __init__(self):
        self.rows, self.made = [], []

    def add(self, x, y, octave, angle, u_right, desc, occupied=0, in_bbox=1, query=-1, flips=-1, what="filler"):
        self.rows.append((F32(x), F32(y), int(octave), F32(angle), F32(u_right), desc, int(occupied), int(in_bbox)))
        self.made.append((query, flips, what))
        return len(self.rows) - 1

    def swap(self, a, b):
        self.rows[a], self.rows[b] = self.rows[b], self.rows[a]
        self.made[a], self.made[b] = self.made[b], self.made[a]

    def side(self, grid):
        n = len(self.rows)
        col = lambda k, dt: np.array([r[k] for r in self.rows], dt) if n else np.zeros(0, dt)
        T = {"x": col(0, F32), "y": col(1, F32), "octave": col(2, np.int32), "angle": col(3, F32), "u_right": col(4, F32),
             "desc": np.array([r[5] for r in self.rows], np.uint8).reshape(n, 32), "occupied": col(6, np.uint8), "in_bbox": col(7, np.uint8),
             "grid": tuple(F32(g) for g in grid)}
        T["cell_off"], T["cell_idx"] = build_grid(T["x"], T["y"], *T["grid"])
        return T


def _blocks_for(nq, nt):
    """(first query, length, trains): consecutive queries that want the same trains; the long ones cross a 64-query block"""
    if nq >= 600 and nt >= 300:
        return ((40, 70, 6), (130, 5, 1), (150, 30, 3), (200, 40, 6), (300, 64, 5), (380, 12, 2), (420, 50, 6), (500, 20, 4))
    if nq >= 129 and nt >= 64:
        return ((30, 70, 6), (110, 12, 2))
    if nq >= 63 and nt >= 63:
        return ((5, 20, 6), (30, 9, 1), (45, 12, 5))
    return ()


def _projection_scene(d, nt, nq, motion, origin, nnratio, plan=None, collide=0, small=False):
    """one searched side with its frame, local-map and object problems.  plan: the frame histogram bin by bin (the first sum(plan)
    queries are lone exact pairs, every other query is invalid); collide: the number of query pairs whose trains are equal modulo 4096"""
    rng = synth.Rng(d.seed(), lanes=1024)
    U = rng.uniform
    w, h = (d.int(200, 260), d.int(120, 160)) if small else (d.int(200, 640), d.int(120, 376))
    bounds, grid, K6 = _camera(d, w, h, origin)
    min_x, max_x, min_y, max_y = [float(v) for v in bounds]
    fx, cx, cy, mb = float(K6[0]), float(K6[2]), float(K6[3]), float(K6[5])
    tcw, tlw = _poses(rng, motion, mb)
    th_frame, th_points = d.pick((3.0, 7.0, 15.0)), d.pick((1.0, 3.0))
    if plan:
        th_frame = 3.0
    R, t = tcw[:3, :3].astype(np.float64), tcw[:3, 3].astype(np.float64)
    # -- where the queries project, and how deep
    where = U(nq)
    if collide:
        where[:2 * collide] = 0.5                               # the colliding queries: inside the image, in front of the camera
    u, v = min_x + U(nq) * w, min_y + U(nq) * h
    side = rng.integers(nq, 0, 8)                              # within a pixel of a bound, inside or outside
    near = (where >= 0.80) & (where < 0.92)
    delta = (U(nq) * 0.98 + 0.01) * np.where(side % 2 == 0, -1.0, 1.0)
    u = np.where(near & (side // 2 == 0), min_x + delta, np.where(near & (side // 2 == 1), max_x + delta, u))
    v = np.where(near & (side // 2 == 2), min_y + delta, np.where(near & (side // 2 == 3), max_y + delta, v))
    u = np.where(where >= 0.96, max_x + 30.0 + 100.0 * U(nq), u)                              # far outside
    zc = 4.0 + 46.0 * U(nq)
    zc = np.where((where >= 0.92) & (where < 0.96), -zc, zc)                                # behind the camera
    level = np.minimum(rng.integers(nq, 0, 8), rng.integers(nq, 0, 8)).astype(np.int32)
    valid = (U(nq) < 0.92).astype(np.uint8)
    observed = (U(nq) < 0.8).astype(np.uint8)
    qdesc = rng.integers(nq * 32, 0, 256).astype(np.uint8).reshape(nq, 32)
    rot = np.round(_rotations(rng, nq) * 2.0) / 2.0 % 360.0                                  # whole and half degrees: exact in float32
    if plan:                                                   # lone pairs on a lattice, 24 pixels apart
        n_pairs = sum(plan)
        per_row = max(1, (w - 30) // 24)
        k = np.arange(nq)
        u = np.where(k < n_pairs, min_x + 15.0 + 24.0 * (k % per_row), u); v = np.where(k < n_pairs, min_y + 15.0 + 24.0 * (k // per_row), v)
        zc = np.where(k < n_pairs, np.abs(zc), zc)
        level[:n_pairs] = 0
        valid = (k < n_pairs).astype(np.uint8)
        bins = np.concatenate([np.full(c, 3 + 7 * b) for b, c in enumerate(plan)])
        rot[:n_pairs] = 12.0 * bins[:min(n_pairs, nq)]
    blocks = () if plan or collide else _blocks_for(nq, nt)
    block_of = np.full(nq, -1)
    for b, (q0, length, _) in enumerate(blocks):
        block_of[q0:q0 + length] = b
        u[q0:q0 + length], v[q0:q0 + length], zc[q0:q0 + length] = min_x + (0.2 + 0.6 * U(1)[0]) * w, min_y + (0.2 + 0.6 * U(1)[0]) * h, 10.0
        level[q0:q0 + length] = int(rng.integers(1, 0, 3)[0])
        qdesc[q0:q0 + length] = qdesc[q0]
        valid[q0:q0 + length] = 1
        observed[q0:q0 + length] = U(length) < 0.7
        observed[q0], observed[q0 + length // 2] = 1, 0        # (both kinds in every block)
    qa, ta = _angle_pair(rng, rot)
    Xc = np.stack([(u - cx) / fx * zc, (v - cy) / fx * zc, zc], 1)
    xw = ((Xc - t) @ R).astype(F32)
    proj = [ms.frame_projection(tcw, K6, xw[i]) for i in range(nq)]
    pu, pv, pur = (np.array([p[k] for p in proj], F32) for k in (1, 2, 3))
    view_cos = (0.99 + 0.01 * U(nq)).astype(F32)
    r_points = np.where(view_cos.astype(np.float64) > 0.998, F32(2.5), F32(4.0)).astype(F32)
    if th_points != 1.0:
        r_points = (r_points * F32(th_points)).astype(F32)
    rer = (r_points * SF[level]).astype(F32)
    # -- the trains: built around each query in turn while rows are left, then fillers
    tr = _Trains()
    room = nt - max(1, nt // 10) if nt > 16 else nt
    recipe = U(nq)
    made = dict(flips=[], ties=[], ratio=[], collisions=[], blocks=blocks)
    pairs = RATIO_PAIRS[nnratio]

    def put(i, k, octave=None, u_right=-1.0, occupied=None, dx=None, what="flip"):
        ox, oy = (U(2) * 4.0 - 2.0) if dx is None else dx
        occ = int(U(1)[0] < 0.05) if occupied is None else occupied
        row = tr.add(pu[i] + F32(ox), pv[i] + F32(oy), level[i] if octave is None else octave, ta[i], u_right, _flipped(rng, qdesc[i:i + 1], [k])[0],
                     occ, int(U(1)[0] < 0.9), i, k, what)
        made["flips"].append((row, i, k))
        return row

    done = set()
    reserved = sum(b[2] for b in blocks)                       # rows kept for the blocks still to come
    for i in range(nq):
        b = block_of[i]
        if b >= 0:
            if b not in done and len(tr.rows) + blocks[b][2] <= room:
                done.add(b)
                reserved -= blocks[b][2]
                for k in BLOCK_DISTANCES[:blocks[b][2]]:
                    put(i, k, occupied=0, what="block")
                    tr.rows[-1] = tr.rows[-1][:7] + (1,)
            continue
        if plan:
            if i < sum(plan) and len(tr.rows) < nt:
                put(i, 0, occupied=0, dx=(0.5, -0.5), what="pair")
                tr.rows[-1] = tr.rows[-1][:7] + (1,)
            continue
        if len(tr.rows) + 4 + reserved > room or not np.isfinite(pu[i]):
            continue
        c = recipe[i]
        if collide and i < 2 * collide:
            put(i, 10, occupied=0, what="collide")
        elif c < 0.08:
            pass
        elif c < 0.38:
            c2 = U(1)[0]                                       # monocular, uR next to the projection, uR far from it
            put(i, d.pick(P_FLIPS), u_right=-1.0 if c2 < 0.6 else float(pur[i]) + U(1)[0] - 0.5 if c2 < 0.85 else abs(float(pur[i])) + 45.0)
        elif c < 0.50:
            k = d.pick((0, 10, 40, 49, 50, 99, 100, 129, 130))
            rows = [put(i, k, occupied=0, what="tie") for _ in range(d.int(2, 4))]
            made["ties"].append((i, k, rows))
        elif c < 0.78:
            best, second = d.pick(pairs)
            best += d.pick((0, 0, -1, 1))
            other = bool(U(1)[0] < 0.45) and level[i] > 0
            order = U(1)[0] < 0.5                                                             # which of the two comes first in the grid
            r1 = put(i, best, occupied=0, dx=(-1.0, 0.5) if order else (1.0, 0.5), what="ratio")
            r2 = put(i, second, octave=level[i] - 1 if other else None, occupied=0, dx=(1.0, 0.5) if order else (-1.0, 0.5), what="ratio")
            made["ratio"].append((i, best, second, other, r1, r2))
        elif c < 0.88:
            up = np.nextafter(rer[i], F32(np.inf)) - rer[i]
            step = (F32(0), np.nextafter(rer[i], F32(0)) - rer[i], up, up, F32(0.5))[d.int(0, 4)]
            put(i, 10, u_right=F32(pur[i] - F32(rer[i] + step)) if U(1)[0] < 0.5 else F32(pur[i] + F32(rer[i] + step)), occupied=0, what="ur")
        else:
            put(i, 10, octave=int(np.clip(level[i] + d.int(-2, 2), 0, 7)), what="level")
    n_built = len(tr.rows)
    while len(tr.rows) < nt:                                                                    # fillers: anywhere, on the bounds, outside the grid
        c = U(4)
        x, y = min_x + c[0] * w, min_y + c[1] * h
        if c[2] < 0.05:
            x, y = (min_x, max_x, x, x)[int(c[3] * 4)], (y, y, min_y, max_y)[int(c[3] * 4)]
        elif c[2] < 0.09:
            x, y = (min_x - 6.0 * c[3] - 0.3 * w / 64, max_x + 6.0 * c[3] + 0.6 * w / 64, x, x)[int(c[3] * 4)], (y, y, min_y - 0.6 * h / 48 - 4 * c[3], max_y + 0.6 * h / 48 + 4 * c[3])[int(c[3] * 4)]
        tr.add(x, y, int(min(rng.integers(2, 0, 8))), 360.0 * U(1)[0], -1.0 if U(1)[0] < 0.5 else x - 20.0 * U(1)[0],
               rng.integers(32, 0, 256).astype(np.uint8), int(U(1)[0] < 0.05), int(U(1)[0] < 0.9))
    for p in range(collide):                                   # query 2p + 1 wants train (train of query 2p) + 4096
        a = next(r for r, (q, _, _) in enumerate(tr.made) if q == 2 * p)
        b = next(r for r, (q, _, _) in enumerate(tr.made) if q == 2 * p + 1)
        tr.swap(b, a + 4096)
        made["collisions"].append((2 * p, 2 * p + 1, a, a + 4096))
        valid[2 * p:2 * p + 2] = 1
    made["flips"] = [(r, q, k) for r, (q, k, what) in enumerate(tr.made) if q >= 0]
    T = tr.side(grid)
    common = {"train": T, "scale_factors": SF}
    frame_q = {"valid": valid, "desc": qdesc, "observed": observed, "angle": qa, "xw": xw, "octave": level}
    points_q = {"valid": valid, "desc": qdesc, "observed": observed, "proj_x": pu, "proj_y": pv, "proj_xr": pur, "level": level, "view_cos": view_cos}
    problems = [dict(common, mode="frame", query=frame_q, tcw=tcw, tlw=tlw, K6=K6, bounds=bounds, th=th_frame, mono=motion == "mono"),
                dict(common, mode="points", query=points_q, th=th_points),
                dict(common, mode="points", query=points_q, th=5.0, object=True)]
    made.update(motion=motion, origin=origin, size=(w, h), n_built=n_built, plan=plan)
    return problems, made


def _dense_window_problem(d, n_dense, n_queries=40):
    """a local-map problem whose queries all project into one spot crowded with n_dense level-0 features: every window holds n_dense
    candidates, more than the everyday key format's 256 (tests/test_match_gpu.py has the over-1024 error case)"""
    rng = synth.Rng(d.seed(), lanes=1024)
    sc = synth.projection_scene(d.seed(), n=n_dense + 300, m=n_queries, w=640, h=376)
    tr = {k: np.array(v) for k, v in sc["train"].items() if k != "grid"}
    tr["grid"] = sc["train"]["grid"]
    tr["x"][:n_dense] = (300 + rng.uniform(n_dense, -3, 3)).astype(F32)
    tr["y"][:n_dense] = (150 + rng.uniform(n_dense, -3, 3)).astype(F32)
    tr["octave"][:n_dense] = 0
    tr["u_right"][:n_dense] = -1
    tr["occupied"][:n_dense] = rng.uniform(n_dense) < 0.03
    tr["cell_off"], tr["cell_idx"] = build_grid(tr["x"], tr["y"], *tr["grid"])
    q = {k: np.array(v) for k, v in sc["points_query"].items()}
    q["proj_x"][:] = 300; q["proj_y"][:] = 150; q["proj_xr"][:] = 250; q["level"][:] = 0; q["view_cos"][:] = 0.9; q["valid"][:] = 1
    q["desc"] = tr["desc"][rng.integers(n_queries, 0, n_dense)].copy()                      # real competition for the same trains
    q["desc"][:, 0] ^= rng.integers(n_queries, 0, 4).astype(np.uint8)
    return {"train": tr, "scale_factors": sc["scale_factors"], "mode": "points", "query": q, "th": 1.0}


def _projection_scenes(d):
    out = []
    for i, (nt, nq) in enumerate(_P_SIZES):
        nnratio = (0.6, 0.8, 0.9)[i % 3]
        probs, made = _projection_scene(d, nt, nq, MOTIONS[i % 4], _P_ORIGIN.get(i, "zero"), nnratio)
        out.append(dict(kind="proj", family="general", nnratio=nnratio, problems=probs, made=[made]))
    for i, ((nt, nq), plan) in enumerate(zip(_HIST_SIZES, HIST_PLANS)):
        probs, made = _projection_scene(d, nt, nq, MOTIONS[(i + 1) % 4], "zero", 0.8, plan=plan, small=True)
        out.append(dict(kind="proj", family="hist", nnratio=0.8, problems=probs, made=[made]))
    for i, nt in enumerate(COLLIDE_TRAIN):
        probs, made = _projection_scene(d, nt, (600, 129)[i], MOTIONS[i], "zero", (0.8, 0.9)[i], collide=(1, 12)[i])
        out.append(dict(kind="proj", family="collide", nnratio=(0.8, 0.9)[i], problems=probs, made=[made]))
    probs, made = _projection_scene(d, 300, 65, "forward", "zero", 0.9)
    out.append(dict(kind="proj", family="wide", nnratio=0.9, problems=[probs[0], _dense_window_problem(d, d.int(300, 700)), probs[1]], made=[made]))
    batch, mades = [], []
    for k in range(65):                                        # 65 problems in one call: 64 threads per problem in pj_resolve, a second group in pj_gather
        nt, nq = d.pick((15, 16, 17, 63, 64)), d.pick((3, 4, 5, 63, 64, 65, 70))
        if k % 13 == 5:
            nq = 0
        if k % 13 == 9:
            nt = 0
        probs, made = _projection_scene(d, nt, nq, MOTIONS[k % 4], ("zero", "negative", "positive")[k % 3], 0.8, small=True)
        batch.append(probs[k % 3]); mades.append(made)
    out.append(dict(kind="proj", family="batch", nnratio=0.8, problems=batch, made=mades))
    return out


# ---- brute-force scenes -------------------------------------------------------------------------------------------------------------
def _bf_problem(d, nq, nt, nnratio, plan=None):
    rng = synth.Rng(d.seed(), lanes=1024)
    U = rng.uniform
    qd = rng.integers(nq * 32, 0, 256).astype(np.uint8).reshape(nq, 32)
    td = rng.integers(nt * 32, 0, 256).astype(np.uint8).reshape(nt, 32)
    rot = np.round(_rotations(rng, nq) * 2.0) / 2.0 % 360.0
    qv = (U(nq) < 0.92).astype(np.uint8)
    made = dict(flips=[], groups=[], collisions=[], ratio=[], plan=plan)
    ladder = BF_LADDER[nnratio]
    # groups of queries with one descriptor, and near-duplicate trains on the ladder: the eight-key lists run out
    groups, q0 = [], 2
    if not plan and nq >= 63:
        for _ in range(nq // 60):
            size, dups = d.int(9, 20), (min(nt, d.int(9, 12)) if nt > 8 else nt)
            if q0 + size <= nq and dups:
                groups.append((q0, size, min(dups, len(ladder))))
            q0 += size + d.int(8, 30)
    group_of = np.full(nq, -1)
    for g, (a, size, _) in enumerate(groups):
        group_of[a:a + size] = g
        qd[a:a + size] = qd[a]
        qv[a:a + size] = 1
    if plan:
        n_pairs = min(sum(plan), nq, nt)
        bins = np.concatenate([np.full(c, 3 + 7 * b) for b, c in enumerate(plan)])
        rot[:n_pairs] = 12.0 * bins[:n_pairs]
        qv = (np.arange(nq) < n_pairs).astype(np.uint8)
    qa, angle_for = _angle_pair(rng, rot)
    ta = (360.0 * U(nt)).astype(F32)
    slots = list(np.argsort(U(nt), kind="stable")) if nt else []                               # a hand-built train takes the next free row of a shuffled order
    pairs = RATIO_PAIRS[nnratio]
    recipe = U(nq)
    neighbours = set()                                         # lanes i, i + 1 of one 64-query chunk whose best trains will be equal modulo 512
    if nt >= 513 and not plan:
        for i in range(24, nq - 1, 5):
            if i % 64 != 63 and group_of[i] < 0 and group_of[i + 1] < 0 and len(neighbours) < 24:
                neighbours |= {i, i + 1}
                qv[i:i + 2] = 1

    def put(i, k, what):
        if not slots:
            return -1
        row = int(slots.pop())
        td[row] = _flipped(rng, qd[i:i + 1], [k])[0]
        ta[row] = angle_for[i]
        made["flips"].append((row, i, k))
        return row

    done = set()
    for i in range(nq):
        g = group_of[i]
        if g >= 0:
            if g not in done:
                done.add(g)
                made["groups"].append((groups[g][0], groups[g][1], [put(i, k, "group") for k in ladder[:groups[g][2]]]))
            continue
        if plan:
            if i < sum(plan):
                put(i, 0, "pair")
            continue
        if i in neighbours:
            put(i, 0, "neighbour")
            continue
        if len(slots) < max(3, nt // 10) + len(neighbours) and nt > 8:
            continue
        c = recipe[i]
        if c < 0.1:
            pass
        elif c < 0.5:
            put(i, d.pick(BF_FLIPS), "flip")
        elif c < 0.62:
            k = d.pick((0, 18, 44, 50))
            for _ in range(d.int(2, 3)):
                put(i, k, "tie")
        else:
            best, second = d.pick(pairs)
            best += d.pick((0, 0, -1, 1))
            made["ratio"].append((i, best, second, put(i, best, "ratio"), put(i, second, "ratio")))
    # neighbouring lanes whose best trains are equal modulo 512
    if nt >= 513 and not plan:
        by_query = {i: row for row, i, k in made["flips"] if i in neighbours}
        for i in sorted(neighbours)[::2]:
            a, b = by_query.get(i), by_query.get(i + 1)
            if a is None or b is None:
                continue
            c = (a + 512) % nt if (a + 512) < nt else a - 512
            if c < 0 or c == b or any(c == r for r, _, _ in made["flips"]):
                continue
            td[[b, c]], ta[[b, c]] = td[[c, b]], ta[[c, b]]
            made["flips"] = [((c if r == b else r), q, k) for r, q, k in made["flips"]]
            by_query[i + 1] = c
            made["collisions"].append((i, i + 1, a, c))
    return {"q_desc": qd, "q_angle": qa, "q_valid": qv, "t_desc": td, "t_angle": ta}, made


def _bf_scenes(d):
    out = []
    for i, shapes in enumerate(_BF_SHAPES):
        nnratio = (0.9, 0.8, 0.6)[i % 3]
        built = [_bf_problem(d, nq, nt, nnratio) for nq, nt in shapes]
        out.append(dict(kind="bf", family="general", nnratio=nnratio, problems=[b[0] for b in built], made=[b[1] for b in built]))
    # many tiny problems in one call: the last free train is a query's only candidate, and then none is left
    built = [_bf_problem(d, (63, 64, 65, 1)[k % 4], (1, 2, 7, 8, 2)[k % 5], 0.8) for k in range(64)]
    out.append(dict(kind="bf", family="tiny", nnratio=0.8, problems=[b[0] for b in built], made=[b[1] for b in built]))
    built = [_bf_problem(d, (64, 65, 63, 130)[k % 4], (255, 256, 257, 511)[k % 4], 0.9, plan=plan) for k, plan in enumerate(HIST_PLANS)]
    out.append(dict(kind="bf", family="hist", nnratio=0.9, problems=[b[0] for b in built], made=[b[1] for b in built]))
    return out


# ---- Fuse scenes ----------------------------------------------------------------------------------------------------------------------
def _fuse_scene(d, n, m, scale=1.2):
    """synth.fuse_scene with n - extra features, then candidates moved onto the gates' boundaries and `extra` features placed around
    other candidates: chi-square just either side of 5.99 / 7.8, descriptors at exactly 50 / 51 bits, ties, one crowded cell.
    scale = 1.1: the keyframe's pyramid has that factor, while the points' distance ranges were made for 1.2 - the predicted level
    leaves 0 .. n_levels - 1 on both sides (at 1.2 the 0.8f / 1.2f distance gate leaves a negative level only on its boundary)"""
    rng = synth.Rng(d.seed(), lanes=1024)
    U = rng.uniform
    extra = 0 if n < 63 or m < 63 else (n // 3 if n < 300 else 150)
    w, h = d.int(200, 640), d.int(120, 376)
    pr = synth.fuse_scene(d.seed(), n=n - extra, m=m, w=w, h=h, th=d.pick((3.0, 5.0)))
    if scale != 1.2:
        sf = np.array([F32(scale) ** k for k in range(8)], F32)
        pr["scale_factors"], pr["inv_level_sigma2"], pr["log_scale_factor"] = sf, (F32(1.0) / (sf * sf)).astype(F32), F32(np.log(F32(scale)))
    q = pr["query"]
    q["valid"] = np.array(q["valid"]); q["desc"] = np.array(q["desc"])
    R, t, ow = pr["R"].astype(np.float64), pr["t"].astype(np.float64), pr["ow"].astype(np.float64)
    T = pr["train"]
    made = dict(flips=[], boundary=[], extra=extra)
    # -- candidates on the boundaries of their own gates
    order = list(np.argsort(U(m), kind="stable"))
    for kind in ("behind", "min_dist", "max_dist", "cosine", "clamp_low", "clamp_high") * (5 if m >= 63 else 0):
        i = int(order.pop())
        q["valid"][i] = 1
        if kind == "behind":
            q["pos"][i] = ((np.array([0.1, 0.1, -1e-4 * (1 + U(1)[0])]) - t) @ R).astype(F32)
        po = q["pos"][i].astype(F32) - pr["ow"].astype(F32)
        dist = F32(math.sqrt(sum(float(c) * float(c) for c in po)))
        nudge = lambda v: (np.nextafter(v, F32(0)), v, np.nextafter(v, F32(np.inf)))[d.int(0, 2)]
        if kind == "min_dist":
            q["min_dist"][i] = nudge(F32(dist / F32(0.8)))
        elif kind == "max_dist":
            q["max_dist"][i] = nudge(F32(dist / F32(1.2))); q["min_dist"][i] = F32(0.01)
        elif kind == "cosine":                                 # 60 degrees +- 1e-4 rad off the viewing ray
            e = po.astype(np.float64) / float(dist)
            side = np.cross(e, [0.0, 1.0, 0.0]); side /= np.linalg.norm(side)
            a = math.pi / 3 + (1e-4 if U(1)[0] < 0.5 else -1e-4)
            q["normal"][i] = (math.cos(a) * e + math.sin(a) * side).astype(F32)
        elif kind == "clamp_low":                              # the ratio on 1 / 1.2f, or inside the gate and below 1 / scale
            q["max_dist"][i] = F32(dist * F32(0.87)) if scale != 1.2 else F32(F32(dist / F32(1.2)) * F32(1 + 2.0 ** -22 * d.int(0, 2)))
            q["min_dist"][i] = F32(0.01)
        elif kind == "clamp_high":
            q["max_dist"][i] = F32(dist * F32(1.2 ** 9)); q["min_dist"][i] = F32(0.01)
        made["boundary"].append((i, kind))
    # -- features around other candidates
    cols = {k: list(np.asarray(T[k])) for k in ("x", "y", "octave", "u_right")}
    descs = list(np.asarray(T["desc"], np.uint8).reshape(-1, 32))

    def put(x, y, octave, u_right, desc):
        cols["x"].append(F32(x)); cols["y"].append(F32(y)); cols["octave"].append(int(octave)); cols["u_right"].append(F32(u_right)); descs.append(desc)
        return len(descs) - 1

    budget = extra - (70 if extra >= 100 else 0)
    kinds = ("chi_mono_in", "chi_mono_out", "chi_stereo_in", "chi_stereo_out", "d50", "d51", "tie")
    turn = 0
    while order and budget >= 2:
        i = int(order.pop())
        geo = ms.fuse_geometry(pr, i) if q["valid"][i] else None
        if geo is None:
            continue
        u, v, ur, lvl, radius = geo
        kind = kinds[turn % len(kinds)]; turn += 1
        q["desc"][i] = rng.integers(32, 0, 256).astype(np.uint8)                             # only the placed features are near this descriptor
        flip = lambda k: _flipped(rng, q["desc"][i:i + 1], [k])[0]
        s = float(pr["scale_factors"][lvl])
        if kind.startswith("chi_mono"):
            e = math.sqrt(5.99) * s * (1 - 2e-3 if kind.endswith("in") else 1 + 2e-3)
            row = put(u + F32(e), v, lvl, -1.0, flip(12)); k = 12
        elif kind.startswith("chi_stereo"):
            e = math.sqrt(7.8 / 3) * s * (1 - 2e-3 if kind.endswith("in") else 1 + 2e-3)
            row = put(u + F32(e), v - F32(e), lvl, F32(ur - F32(e)), flip(12)); k = 12
        elif kind == "tie":
            put(u + F32(0.25), v, lvl, -1.0, flip(20)); budget -= 1; made["flips"].append((len(descs) - 1, i, 20))
            row = put(u, v + F32(0.25), lvl, -1.0, flip(20)); k = 20
        else:
            k = 50 if kind == "d50" else 51
            row = put(u + F32(0.25), v - F32(0.25), lvl, -1.0, flip(k))
        made["flips"].append((row, i, k))
        budget -= 1
    crowd = None
    while len(descs) < n:                                      # the rest: one crowded cell (the inner 64-lane chunk), then anywhere
        if crowd is None:                                      # where a candidate that passes its own gates looks
            geo = next((g for g in (ms.fuse_geometry(pr, i) for i in range(m) if q["valid"][i]) if g is not None), None)
            cw, ch = w / 64.0, h / 48.0                        # ... the middle of that cell
            crowd = (w / 2, h / 2) if geo is None else (round(float(geo[0]) / cw) * cw, round(float(geo[1]) / ch) * ch)
        c = U(2)
        put(crowd[0] + 1.8 * c[0] - 0.9, crowd[1] + 1.8 * c[1] - 0.9, int(rng.integers(1, 0, 4)[0]), -1.0, rng.integers(32, 0, 256).astype(np.uint8))
    made["crowd"] = crowd
    T = {"x": np.array(cols["x"], F32), "y": np.array(cols["y"], F32), "octave": np.array(cols["octave"], np.int32), "u_right": np.array(cols["u_right"], F32),
         "desc": np.array(descs, np.uint8).reshape(-1, 32), "grid": (F32(0), F32(0), F32(64) / F32(w), F32(48) / F32(h))}
    T["cell_off"], T["cell_idx"] = build_grid(T["x"], T["y"], *T["grid"])
    pr["train"] = T
    # -- the bounds: through one candidate's u (`u < maxX` fails on it) and another one's v (`v >= minY` holds on it)
    pr["bounds"] = (0.0, float(w), 0.0, float(h))
    geos = [(i, ms.fuse_geometry(pr, i)) for i in range(m) if q["valid"][i]]
    inside = [(i, g) for i, g in geos if g is not None]
    if len(inside) >= 20:
        us, vs = sorted(float(g[0]) for _, g in inside), sorted(float(g[1]) for _, g in inside)
        pr["bounds"] = (0.0, us[-max(2, len(us) // 20)], vs[max(1, len(vs) // 20)], float(h))
        made["bounds_from"] = True
    return pr, made


def _fuse_scenes(d):
    out = []
    for k in range(0, len(_F_SIZES), 3):
        built = [_fuse_scene(d, n, m, 1.1 if (n, m) in _F_SIZES[-2:] else 1.2) for n, m in _F_SIZES[k:k + 3]]
        out.append(dict(kind="fuse", family="general", nnratio=0.8, problems=[b[0] for b in built], made=[b[1] for b in built]))
    return out


@functools.lru_cache(maxsize=None)
def scenes(seed, budget):
    """the first `budget` calls of the run: projection, brute-force and Fuse scenes interleaved so that a larger scene's scratch lies
    under a smaller later one.  The arrays are shared: do not write into them."""
    d = sweep_cases._Draw(int(seed))
    proj, bf, fuse = _projection_scenes(d), _bf_scenes(d), _fuse_scenes(d)
    out = []
    while proj or bf or fuse:
        for family in (proj, bf, proj, fuse, proj):
            if family:
                out.append(family.pop(0))
    return out[:int(budget)]


# ---- the references ------------------------------------------------------------------------------------------------------------------
def mode_of(scene, pr):
    return scene["kind"] if scene["kind"] != "proj" else ("frame" if pr["mode"] == "frame" else "object" if pr.get("object") else "points")


def oracle_answer(scene, pr, check_ori):
    mode = mode_of(scene, pr)
    if mode == "frame":
        return oracle_lib.search_projection_frame(pr, check_ori)
    if mode in ("points", "object"):
        return oracle_lib.search_projection_points(pr, scene["nnratio"])
    if mode == "bf":
        return oracle_lib.search_bruteforce(pr, scene["nnratio"], check_ori)
    return oracle_lib.fuse_search(pr)


def second_opinion(scene, pr, check_ori, counts=None):
    mode = mode_of(scene, pr)
    if mode == "frame":
        return ms.search_by_projection_frame(pr, check_ori, accumulate="double", counts=counts)
    if mode in ("points", "object"):
        return ms.search_by_projection_points(pr, scene["nnratio"], obj=mode == "object", counts=counts)
    if mode == "bf":
        return ms.search_by_bruce_matching(pr, scene["nnratio"], check_ori, counts=counts)
    return ms.fuse_search(pr, counts=counts)


def reference_of(scene):
    """per problem: dict(mode, oracle = {check_ori: answer}, second = {check_ori: answer}, counts = the gates of the check_ori run).
    Only the frame and brute-force answers depend on check_ori; the others are computed once."""
    out = []
    for pr in scene["problems"]:
        mode = mode_of(scene, pr)
        counts = {}
        ref = dict(mode=mode, counts=counts, oracle={True: oracle_answer(scene, pr, True)}, second={True: second_opinion(scene, pr, True, counts)})
        if mode in ("frame", "bf"):
            ref["oracle"][False], ref["second"][False] = oracle_answer(scene, pr, False), second_opinion(scene, pr, False)
        else:
            ref["oracle"][False], ref["second"][False] = ref["oracle"][True], ref["second"][True]
        out.append(ref)
    return out


@functools.lru_cache(maxsize=None)
def references(seed, budget):
    """reference_of every scene, computed once per process"""
    return [reference_of(s) for s in scenes(seed, budget)]


def totals_of(refs):
    """{mode: {gate: times passed}} over a run's references"""
    tot = {m: {} for m in MODES}
    for ref in refs:
        for r in ref:
            for g, c in r["counts"].items():
                tot[r["mode"]][g] = tot[r["mode"]].get(g, 0) + c
    return tot


def counts_line(totals):
    """the totals of a run as the module's docstring states them: one paragraph per mode, gates in alphabetical order"""
    return "\n".join("    %s: %s" % (m, ", ".join("%s %d" % (g, totals[m][g]) for g in sorted(totals[m]))) for m in MODES)


# ---- the random scenes tools/stress_matchers.py has always drawn ---------------------------------------------------------------------
def _tool():
    """tools/stress_matchers.py as a module: it owns the draw order of its random scenes (random_scenes, random_scene_problems)"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "stress_matchers.py")
    spec = importlib.util.spec_from_file_location("stress_matchers", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def windows_over_1024(probs, nnratio):
    """how many search windows of a call's projection problems hold more than 1024 candidates, by the second opinion's count: such
    a call ends with the documented capacity error"""
    counts = {}
    for pr in probs:
        second_opinion(dict(kind="proj", nnratio=nnratio), pr, True, counts)
    return counts.get("over_1024_candidates", 0)


def random_run_totals(seed=20250503, nscenes=60):
    """the gates the tool's random run passes, under the counters of the committed scenes (check_ori and that call's nnratio; 0.9 for
    the brute-force problem, as the tool calls it)"""
    refs = []
    tool = _tool()
    for s in tool.random_scenes(seed, nscenes):
        probs, bp, fs = tool.random_scene_problems(s)
        for scene, prs in ((dict(kind="proj", nnratio=s["ratios"][True]), probs), (dict(kind="bf", nnratio=0.9), [bp]), (dict(kind="fuse", nnratio=0.9), [fs])):
            ref = []
            for pr in prs:
                counts = {}
                second_opinion(scene, pr, True, counts)
                ref.append(dict(mode=mode_of(scene, pr), counts=counts))
            refs.append(ref)
    return totals_of(refs)
