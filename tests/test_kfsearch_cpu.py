"""CPU checks around ps_kf_search / ps_search_by_sim3: the numpy second opinion (tests/kfsearch_second_opinion.py) on the cases whose
answers are known by construction, what every seeded case of the GPU file is named for, the input condition of the GPU comparison,
and the presence of the C-ABI."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import kfsearch_cases as kc
import kfsearch_second_opinion as so
import sweep_cases

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(kc.KF_BUILDERS) + sorted(kc.SIM3_BUILDERS)


@pytest.mark.parametrize("mode", [0, 2])
def test_second_opinion_on_the_contention_case(mode):
    """answers listed by construction: who gets the contested slot, who falls back to a second candidate under the threshold, who is
    left with one over it, and the slot occupied at entry"""
    pr, ref = kc.problem("contention_%d" % mode), kc.reference("contention_%d" % mode)
    for slot, point in pr["expect"].items():
        assert ref["match_of_train"][slot] == point, (slot, point, ref["match_of_train"][:8])
    for p in pr["expect_unmatched"]:
        assert p not in ref["match_of_train"].tolist() and ref["gate"][p] == "nomatch"
    assert ref["nmatches"] == 4 and (ref["match_of_train"][6:] == -1).all()
    assert pr["train"]["occupied"].sum() == 1


def test_second_opinion_first_in_traversal_order_wins():
    """two features at the same distance: the one in the earlier grid column wins although its index is the higher one"""
    for mode in (0, 1, 2):
        pr, ref = kc.problem("tie_%d" % mode), kc.reference("tie_%d" % mode)
        assert len(pr["expect_tie"]) == 6
        for p, left, right in pr["expect_tie"]:
            assert left > right
            if mode == 1:
                assert ref["best_idx"][p] == left and ref["best_dist"][p] == 5
            else:
                assert ref["match_of_train"][left] == p and ref["match_of_train"][right] == -1
    pr, ref = kc.problem("sim3_tie"), kc.reference("sim3_tie")
    assert len(pr["expect_tie"]) >= 3
    for i1, left, right in pr["expect_tie"]:
        assert left > right and ref["match1"][i1] == left and ref["match2"][left] == i1 and ref["match12"][i1] == left


def test_quirks_of_the_relocalisation_overload_are_pinned():
    p, f = kc.problem("behind_2")["expect_behind"]
    assert kc.reference("behind_2")["match_of_train"][f] == p
    assert kc.reference("behind_0")["gate"][p] == "depth" and kc.reference("behind_0")["match_of_train"][f] == -1
    p, f = kc.problem("edge_2")["expect_edge"]
    assert kc.reference("edge_2")["match_of_train"][f] == p
    assert kc.reference("edge_0")["gate"][p] == "image" and kc.reference("edge_1")["gate"][p] == "image"
    assert kc.reference("edge_1")["best_idx"][p] == -1 and kc.reference("edge_1")["best_dist"][p] == 256
    # the point behind the camera of main_2 is searched as well
    assert "depth" not in kc.reference("main_2")["gate"]


def test_rot13_pins_the_histogram_factor():
    """1.0f / HISTO_LENGTH puts every match into bins 0 .. 12; the tracking overloads' HISTO_LENGTH / 360.0f would give another result"""
    pr, ref = kc.problem("rot13"), kc.reference("rot13")
    bins = ref["bins"]
    assert all(b > 0 for b in bins[:13]) and not any(bins[13:])
    assert (ref["match_of_train"] == -2).sum() >= 20 and ref["nmatches"] >= 20
    other = so.search_by_projection_keyframe(pr, True, factor=F32(so.HISTO_LENGTH) / F32(360.0))
    assert any(other["bins"][13:])
    assert not np.array_equal(other["match_of_train"], ref["match_of_train"]) and other["nmatches"] != ref["nmatches"]
    assert (kc.reference("main_2")["match_of_train"] == -2).any()


def test_seeded_cases_cover_what_they_are_named_for():
    for mode, names in ((0, ("main_0",)), (1, ("main_1",)), (2, ("main_2", "main_2_64"))):
        for name in names:
            assert set(kc.reference(name)["gate"]) == set(so.GATES[mode]), name
    for name in ("sim3_main", "sim3_main_093"):
        pr, ref = kc.problem(name), kc.reference(name)
        assert set(ref["gate"]) == set(so.GATES[3]), name
        n1 = len(pr["kf1"]["x"])
        assert n1 == len(pr["kf2"]["x"]) == 500 and 250 <= pr["kf1"]["has_point"].sum() <= 400
        assert pr["kf1"]["already"].sum() == 40 and pr["kf2"]["already"].sum() == 40
        assert (ref["match12"][pr["kf1"]["already"] > 0] == -1).all()
        one_way = (ref["match1"] >= 0) & (ref["match12"] < 0)
        assert ref["nfound"] >= 50 and one_way.sum() >= 10
        assert pr["kf2"]["K4"][0] != pr["kf1"]["K4"][0] and pr["K4"] == pr["kf1"]["K4"]
    # descriptor distances straddle the thresholds 50, 64 and 100
    for name, lo, hi in (("main_1", 50, 50),):
        bd = kc.reference(name)["best_dist"]
        assert (bd <= lo).any() and ((bd > hi) & (bd < 256)).any()
    # occupied slots at entry, and assignments that depend on the order
    for name in ("main_0", "main_2", "contention_0", "contention_2", "wide_0", "wide_2"):
        assert kc.problem(name)["train"]["occupied"].any(), name
    # the wide cases: more takeable candidates in a window than the everyday store keeps
    for name in ("wide_0", "wide_2"):
        pr = kc.problem(name)
        assert len(pr["train"]["x"]) == 340 and kc.reference(name)["nmatches"] == 12
    big = kc.over()
    assert [len(p["train"]["x"]) for p in big] == [120, 8192, 120]
    assert len(kc.problem("empty_nq_0")["query"]["valid"]) == 0 and len(kc.problem("empty_n_2")["train"]["x"]) == 0
    assert sorted({kc.problem(n)["mode"] for n in kc.BATCH}) == [0, 1, 2] and len(kc.BATCH) == 16


@pytest.mark.parametrize("name", ALL)
def test_input_condition_of_the_gpu_comparison(name):
    """PredictScale is the one libm-dependent quantity of these members.  For every query of every seeded case the predicted level
    is unchanged when log(ratio) / logScale moves by +- 4 ulp in FP64, and ratio is not within 4 float ulp of a power of 1.2: two
    correctly working implementations cannot disagree on a level.  No query is excluded."""
    ref = kc.reference(name)
    lv = ref["logv"][np.isfinite(ref["logv"])]
    assert np.isfinite(ref["logv"]).sum() == sum(g in ("empty", "nomatch", "match") for g in ref["gate"])
    assert sweep_cases.level_violations(ref) == (0, len(lv))       # the predicate itself: one statement, shared with the sweeps


def test_decomposition_helpers_state_their_model():
    from pointslot_amd.matcher import decompose_scw, sim3_pair
    rng = np.random.RandomState(3)
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = 0.93 * R, 0.93 * rng.normal(size=3)
    S = S.astype(F32)
    Rcw, tcw, ow, scw = decompose_scw(S)
    assert Rcw.dtype == tcw.dtype == ow.dtype == F32
    assert scw == F32(math.sqrt(sum(float(v) * float(v) for v in S[0, :3])))
    assert np.array_equal(Rcw, (S[:3, :3].astype(np.float64) * (1.0 / float(scw))).astype(F32))
    assert np.allclose(Rcw.astype(np.float64) @ Rcw.astype(np.float64).T, np.eye(3), atol=1e-6)
    assert np.allclose(ow, -(Rcw.astype(np.float64).T @ tcw.astype(np.float64)), atol=1e-6)
    sr12, t12, sr21, t21 = sim3_pair(F32(0.93), R, [1, 2, 3])
    assert np.allclose(sr12.astype(np.float64) @ sr21.astype(np.float64), np.eye(3), atol=1e-6)
    assert np.allclose(sr12.astype(np.float64) @ t21.astype(np.float64) + t12, 0, atol=1e-5)


def test_abi_has_the_keyframe_searches(tmp_path):
    """the four symbols resolve in libpointslot_hip.so, and sizeof / offsetof of the new structs, printed by a C program, equal the
    ctypes mirrors"""
    lib = os.path.join(ROOT, "pointslot_amd", "libpointslot_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ("ps_kf_search", "ps_kf_search_frames", "ps_search_by_sim3", "ps_search_by_sim3_frames"):
        assert any(line.split()[-1] == name for line in syms.splitlines() if line.strip()), name
    from pointslot_amd import matcher
    K, S, P = matcher._KfSearchProblem, matcher._Sim3Side, matcher._Sim3Problem
    mine = [ctypes.sizeof(K), K.mode.offset, K.q_angle.offset, K.bounds.offset, K.th_dist.offset, K.match_of_train.offset, K.nmatches.offset,
            ctypes.sizeof(S), S.has_point.offset, S.rcw.offset, S.n_levels.offset,
            ctypes.sizeof(P), P.kf2.offset, P.fx.offset, P.sr21.offset, P.th.offset, P.match12.offset, P.nfound.offset]
    exe = str(tmp_path / "kfsearch_abi_sizes")
    fields = ["sizeof(ps_kf_search_problem)"] + ["offsetof(ps_kf_search_problem, %s)" % f for f in ("mode", "q_angle", "bounds", "th_dist", "match_of_train", "nmatches")]
    fields += ["sizeof(ps_sim3_side)"] + ["offsetof(ps_sim3_side, %s)" % f for f in ("has_point", "rcw", "n_levels")]
    fields += ["sizeof(ps_sim3_problem)"] + ["offsetof(ps_sim3_problem, %s)" % f for f in ("kf2", "fx", "sr21", "th", "match12", "nfound")]
    with open(exe + ".c", "w") as f:
        f.write('#include "pointslot_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { size_t v[] = {%s}; '
                'for (unsigned i = 0; i < sizeof v / sizeof *v; i++) printf("%%zu ", v[i]); return 0; }\n' % ", ".join(fields))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), exe + ".c", "-o", exe])
    assert [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()] == mine


def test_cpp_and_python_state_the_same_decomposition_model(tmp_path):
    """ORBmatcher::DecomposeScw / Sim3Pair of the C++ shim and matcher.decompose_scw / sim3_pair give the same floats bit for bit"""
    from pointslot_amd.matcher import decompose_scw, sim3_pair
    rng = np.random.RandomState(9)
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = 1.07 * R, rng.normal(size=3) * 3
    S, R12, t12, s12 = S.astype(F32), R.astype(F32), rng.normal(size=3).astype(F32), F32(0.93)
    lit = lambda a: ", ".join("%sf" % float(v).hex() for v in np.asarray(a, F32).ravel())
    exe = str(tmp_path / "decompose_check")
    with open(exe + ".cpp", "w") as f:
        f.write('#include <cstdio>\n#include <cstring>\n#include "ORBmatcher.h"\n'
                'static void put(const float* v, int n) { for (int i = 0; i < n; i++) { unsigned u; std::memcpy(&u, v + i, 4); std::printf("%%08x ", u); } }\n'
                'int main() { const float s[16] = {%s}, r[9] = {%s}, t[3] = {%s}; pscv::Mat S(4, 4, pscv::CV_32F), R(3, 3, pscv::CV_32F), T(3, 1, pscv::CV_32F);\n'
                '  std::memcpy(S.data, s, 64); std::memcpy(R.data, r, 36); std::memcpy(T.data, t, 12);\n'
                '  float rcw[9], tcw[3], ow[3], a[9], b[3], c[9], d[3];\n'
                '  ORB_SLAM2::ORBmatcher::DecomposeScw(S, rcw, tcw, ow); ORB_SLAM2::ORBmatcher::Sim3Pair(%sf, R, T, a, b, c, d);\n'
                '  put(rcw, 9); put(tcw, 3); put(ow, 3); put(a, 9); put(b, 3); put(c, 9); put(d, 3); return 0; }\n' % (lit(S), lit(R12), lit(t12), float(s12).hex()))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pointslot_amd", "host"), "-I", os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe,
                           "-L", os.path.join(ROOT, "pointslot_amd"), "-lpointslot_hip", "-Wl,-rpath," + os.path.join(ROOT, "pointslot_amd"), "-Wl,-rpath-link,/opt/rocm/lib"])
    got = np.array([int(v, 16) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()], np.uint32)
    Rcw, tcw, ow, _ = decompose_scw(S)
    want = np.concatenate([np.asarray(v, F32).ravel() for v in (Rcw, tcw, ow) + tuple(sim3_pair(s12, R12, t12))]).view(np.uint32)
    assert np.array_equal(got, want), (got, want)


def test_searched_side_packing_under_the_host_sanitizers(tmp_path):
    """tests/cpp/search_side_check.cpp over pointslot_amd/csrc/search_side.h (a stand-alone program; nothing loaded into Python is
    sanitized): the arena stride, the projection / fuse / kf_search layouts with skip ranges that are exactly the staged slots, and
    side_pack on sides of 3, 0 and 2 features - the last with a grid that claims 5 entries over a cell_idx of exactly 2 - byte for
    byte against values written out by hand, nothing touched outside the slices, no report from either sanitizer."""
    exe = str(tmp_path / "search_side_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "pointslot_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "search_side_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1].startswith("ok ") and "FAILED" not in out.stdout, out.stdout
