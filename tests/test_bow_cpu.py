"""CPU checks around the bag-of-words calls: the second opinion (tests/bow_second_opinion.py) on hand-built cases whose answers
are known by construction, the input conditions of every seeded case the GPU file uses, the presence of the C-ABI, and the
host-only vocabulary file parser under the host sanitizers (a stand-alone program; nothing loaded into Python is sanitized)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bow_cases
import bow_second_opinion as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _so_vocab(v):
    return so.Vocab(v["k"], v["L"], v["weighting"], v["parent"], v["desc"], v["weight"], v["is_leaf"])


@pytest.mark.parametrize("weighting", [so.TF_IDF, so.TF, so.IDF, so.BINARY])
def test_second_opinion_on_the_hand_built_vocabulary(weighting):
    """sibling tie (features 1 and 6), stopped word (2), shallow leaves (3, 4), a repeated word (0 and 5), levelsup >= L"""
    voc = _so_vocab(bow_cases.hand_vocabulary(weighting))
    assert voc.nwords == 17
    raw = np.array(bow_cases.HAND_BOW_VALUES[weighting])
    for levelsup, nodes in bow_cases.HAND_NODES.items():
        word, node, ids, vals = voc.transform(bow_cases.HAND_FEATURES, levelsup)
        assert word.tolist() == bow_cases.HAND_WORDS
        assert node.tolist() == nodes, levelsup
        assert ids.tolist() == bow_cases.HAND_BOW_IDS
        assert np.array_equal(vals, raw / raw.sum())      # (all values and their sum are exact in binary)


def test_second_opinion_leaves_a_shallow_leafs_node_unwritten():
    """the reference never writes *nid for a leaf above the asked level; the second opinion reports that as None"""
    voc = _so_vocab(bow_cases.hand_vocabulary())
    assert voc.transform_one(bow_cases.HAND_FEATURES[3], 0)[2] is None
    assert voc.transform_one(bow_cases.HAND_FEATURES[3], 2)[2] == 3
    assert voc.transform_one(bow_cases.HAND_FEATURES[4], 0)[2] is None


@pytest.mark.parametrize("mode", [0, 1])
def test_second_opinion_on_the_hand_built_search(mode):
    a, b, want = bow_cases.hand_search()
    n, match = so.search_by_bow(a, b, mode, 0.9, 1)
    expect = np.full(len(match), -1, np.int32)
    for i, v in want[mode].items():
        expect[i] = v
    assert match.tolist() == expect.tolist()
    assert n == len(want[mode])
    # the 50 / 51 pair shows the `<=` of the first overload against the `<` of the second
    assert len(want[0]) == len(want[1]) + 2
    # without the rotation check the lone fourth bin survives
    assert so.search_by_bow(a, b, mode, 0.9, 0)[0] == n + 1
    # without the skip rule the second feature of the "taken" node goes to the candidate its predecessor holds
    _, loose = so.search_by_bow(a, b, mode, 0.9, 1, skip_rule=False)
    assert not np.array_equal(loose, match)


@pytest.mark.parametrize("name", sorted(bow_cases.FAMILY_CASES))
@pytest.mark.parametrize("mode", [0, 1])
def test_seeded_search_cases_exercise_the_rules(name, mode):
    """What makes a family case a test: the reference's own gate of 15 matches (Tracking.cc:2941) under every setting, at
    least one entry that the already-matched rule changes, at least one that the ratio decides."""
    for ori in (0, 1):
        for ratio in (0.7, 0.9):
            assert bow_cases.family_reference(name, mode, ori, ratio)[0] >= 15
    m7, m9 = bow_cases.family_reference(name, mode, 0, 0.7)[1], bow_cases.family_reference(name, mode, 0, 0.9)[1]
    assert int((m7 != m9).sum()) >= 1
    for ratio in (0.7, 0.9):
        loose = bow_cases.family_reference(name, mode, 0, ratio, False)[1]
        assert int((loose != bow_cases.family_reference(name, mode, 0, ratio)[1]).sum()) >= 1


def test_seeded_transform_cases_cover_what_they_are_named_for():
    v = bow_cases.vocabulary("pruned_k3_L6")
    leaf_depths = set(v["depth"][v["is_leaf"] != 0].tolist())
    assert len(leaf_depths) >= 4                                   # leaves at several depths
    assert int(((v["is_leaf"] != 0) & (v["weight"] <= 0)).sum()) >= 5
    word, node, ids, vals = bow_cases.transform_reference("pruned_k3_L6", 0)
    assert (word < 0).any() and (word >= 0).sum() > 50
    assert np.array_equal(bow_cases.transform_reference("pruned_k3_L6", 9)[1] >= 0, word >= 0)
    assert set(bow_cases.transform_reference("pruned_k3_L6", 9)[1].tolist()) <= {0, -1}
    # sibling pairs with one descriptor; a third of the features are copies of node descriptors, so some land on such a pair
    voc = bow_cases.second_opinion_vocabulary("pruned_k3_L6")
    tied_nodes = sum(1 for ch in voc.children if len(ch) > 1 and np.array_equal(voc.descriptor[ch[0]], voc.descriptor[ch[1]]))
    assert tied_nodes >= 10
    assert bow_cases.vocabulary("wide_k20_L2")["k"] > 16           # a second pass over the 16-lane row
    assert abs(vals.sum() - 1.0) < 1e-12


def test_synthetic_vocabulary_round_trips_through_the_file(tmp_path):
    from pointslot_amd import bow
    v = bow_cases.vocabulary("pruned_k3_L6")
    path = str(tmp_path / "voc.bin")
    bow.save_binary(path, v["k"], v["L"], v["weighting"], v["parent"], v["desc"], v["weight"], v["is_leaf"])
    assert os.path.getsize(path) == 24 + 41 * len(v["parent"])


def test_descriptor_families_leave_the_default_generator_alone():
    from pointslot_amd import keyframes
    plain = keyframes.keyframe_set(5, n_kf=2, n=60)
    again = keyframes.keyframe_set(5, n_kf=2, n=60, descriptor_families=None)
    fam = keyframes.keyframe_set(5, n_kf=2, n=60, descriptor_families=(5, 4, 8))
    for k in ("x", "desc", "node", "angle"):
        assert np.array_equal(plain[0][k], again[0][k])
    assert np.array_equal(plain[0]["x"], fam[0]["x"]) and not np.array_equal(plain[0]["desc"], fam[0]["desc"])


def test_abi_has_the_bag_of_words_calls(tmp_path):
    lib = ctypes.CDLL(os.path.join(ROOT, "pointslot_amd", "libpointslot_hip.so"))
    for name in ("ps_vocabulary_create", "ps_vocabulary_load_binary", "ps_vocabulary_destroy", "ps_vocabulary_info", "ps_bow_transform",
                 "ps_search_by_bow"):
        assert getattr(lib, name) is not None
    from pointslot_amd import bow, matcher
    assert ctypes.sizeof(bow._BowProblem) == 64 and ctypes.sizeof(matcher._BowSide) == 40 and ctypes.sizeof(matcher._BowSearchProblem) == 112
    exe = str(tmp_path / "bow_abi_sizes")
    with open(exe + ".c", "w") as f:
        f.write('#include "pointslot_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ps_bow_problem), '
                'sizeof(ps_bow_side), sizeof(ps_bow_search_problem), offsetof(ps_bow_problem, bow_n), offsetof(ps_bow_search_problem, match)); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), exe + ".c", "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["64", "40", "112", "56", "96"]


def test_vocabulary_file_parser_under_the_host_sanitizers(tmp_path):
    """tests/cpp/vocab_file_check.cpp over pointslot_amd/csrc/vocab_file.h: round trip of a file written by save_binary, clean
    errors for a truncated file, size_node != 41, a record count that disagrees with the file length, parents out of range -
    and no report from AddressSanitizer / UndefinedBehaviorSanitizer."""
    from pointslot_amd import bow
    v = bow_cases.vocabulary("pruned_k3_L6")
    good = str(tmp_path / "good.bin")
    bow.save_binary(good, v["k"], v["L"], v["weighting"], v["parent"], v["desc"], v["weight"], v["is_leaf"])
    raw = open(good, "rb").read()
    n = len(v["parent"])

    def write(name, data):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        return p
    import struct
    truncated = write("truncated.bin", raw[:24 + 41 * (n // 2) + 7])
    short_head = write("short_head.bin", raw[:10])
    size40 = write("size40.bin", raw[:4] + struct.pack("<I", 40) + raw[8:])
    more = write("more.bin", struct.pack("<I", n + 3) + raw[4:])
    fewer = write("fewer.bin", struct.pack("<I", n - 3) + raw[4:])
    bad_parent = bytearray(raw)
    bad_parent[24 + 41 * 5:24 + 41 * 5 + 4] = struct.pack("<i", 1000000)
    forward = write("forward.bin", bytes(bad_parent))
    bad_parent[24 + 41 * 5:24 + 41 * 5 + 4] = struct.pack("<i", -2)
    negative = write("negative.bin", bytes(bad_parent))
    exe = str(tmp_path / "vocab_file_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "pointslot_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "vocab_file_check.cpp"), "-o", exe])
    leaf = v["is_leaf"] != 0
    wsum = float(np.asarray(v["weight"], np.float64).sum())
    out = subprocess.run([exe, good, str(n), str(int(leaf.sum())), "%.17g" % wsum, str(int(v["parent"].astype(np.int64).sum())),
                          str(int(v["desc"].astype(np.int64).sum())), truncated, short_head, size40, more, fewer, forward, negative],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "ok 8 checks", out.stdout
