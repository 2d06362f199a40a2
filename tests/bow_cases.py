"""The seeded and hand-built cases of the bag-of-words tests (tests/test_bow_cpu.py checks their input conditions on the CPU,
tests/test_bow_gpu.py runs them on the device) and their second-opinion answers, computed once per process."""
import functools

import numpy as np

import bow_second_opinion as so
from pointslot_amd import bow, keyframes, synth

F32 = np.float32


def ones(n):
    """a 32-byte descriptor with its first n bits set: distance(ones(a), ones(b)) = |a - b|"""
    bits = np.zeros(256, np.uint8)
    bits[:n] = 1
    return np.packbits(bits)


def flipped(d, positions):
    bits = np.unpackbits(np.asarray(d, np.uint8))
    bits[list(positions)] ^= 1
    return np.packbits(bits)


# ---- the hand-built vocabulary: k = 3, L = 3 ---------------------------------------------------------------------------------
def hand_vocabulary(weighting=so.TF_IDF):
    """Nodes in record order (node id = record + 1).  Level 1: 1, 2 inner, 3 a leaf (depth 1).  Level 2: 4, 5, 6 under 1 (5 and 6
    carry the same descriptor: a tie), 7, 8 under 2 inner and 9 a leaf (depth 2).  Level 3: three leaves under each of 4 .. 8
    (22 and 23 are equally far from the probe of feature 6).  Words in leaf-record order: node 3 -> 0, node 9 -> 1, nodes
    10 .. 24 -> 2 .. 16; weight(word) = 1 + word / 2, except word 12 (node 20), which is stopped."""
    rows = [(0, 0, 0), (0, 100, 0), (0, 200, 1),                       # 1 2 3
            (1, 0, 0), (1, 20, 0), (1, 20, 0), (2, 90, 0), (2, 100, 0), (2, 110, 1),   # 4 .. 9
            (4, 0, 1), (4, 3, 1), (4, 6, 1), (5, 18, 1), (5, 20, 1), (5, 22, 1), (6, 18, 1), (6, 20, 1), (6, 22, 1),
            (7, 88, 1), (7, 90, 1), (7, 92, 1), (8, 98, 1), (8, 100, 1), (8, 102, 1)]
    parent = np.array([r[0] for r in rows], np.int32)
    desc = np.stack([ones(r[1]) for r in rows])
    leaf = np.array([r[2] for r in rows], np.uint8)
    weight = np.zeros(len(rows), F32)
    w = 0
    for i in range(len(rows)):
        if leaf[i]:
            weight[i] = 0.0 if w == 12 else 1.0 + 0.5 * w
            w += 1
    return dict(k=3, L=3, weighting=weighting, parent=parent, desc=desc, weight=weight, is_leaf=leaf)


HAND_FEATURES = np.stack([ones(n) for n in (1, 20, 90, 210, 111, 1, 99)])
HAND_WORDS = [2, 6, -1, 0, 1, 2, 14]
HAND_NODES = {0: [10, 14, -1, 3, 9, 10, 22], 1: [4, 5, -1, 3, 9, 4, 8], 2: [1, 1, -1, 3, 2, 1, 2], 3: [0, 0, -1, 0, 0, 0, 0],
              5: [0, 0, -1, 0, 0, 0, 0]}
HAND_BOW_IDS = [0, 1, 2, 6, 14]
HAND_BOW_VALUES = {so.TF_IDF: [1.0, 1.5, 4.0, 4.0, 8.0], so.TF: [1.0, 1.5, 4.0, 4.0, 8.0], so.IDF: [1.0, 1.5, 2.0, 4.0, 8.0],
                   so.BINARY: [1.0, 1.5, 2.0, 4.0, 8.0]}      # before the L1 normalisation


# ---- the hand-built search case: one feature pair per exit -----------------------------------------------------------------------
def hand_search():
    """Every sub-case sits in a vocabulary node of its own.  Returns (a, b, want): want[mode] = {index of the match array: value}
    with nn_ratio 0.9 and the rotation check on; every other entry is -1."""
    rng = np.random.RandomState(3)
    base = lambda: rng.randint(0, 256, 32).astype(np.uint8)
    A, B = [], []          # rows (desc, angle, node, has_point)

    def add(side, desc, angle, node, has_point=1):
        side.append((desc, angle, node, has_point))
        return len(side) - 1
    want0, want1 = {}, {}

    def pair(da, db, rot, node, in0=True, in1=True, pa=1, pb=1):
        ia, ib = add(A, da, float(rot), node, pa), add(B, db, 0.0, node, pb)
        if in0:
            want0[ib] = ia
        if in1:
            want1[ia] = ib
        return ia, ib
    x = base(); pair(x, x, 0, 10, in0=False, in1=False, pa=0)                      # no point on side a
    y = base()                                                                     # taken by an earlier feature
    ia1, ib1 = pair(y, y, 0, 20)
    ia2 = add(A, flipped(y, [0, 1]), 0.0, 20); ib2 = add(B, flipped(y, range(2, 42)), 0.0, 20)   # 2 from b1, 42 (40 + 2) from b2
    want0[ib2] = ia2; want1[ia2] = ib2
    z = base(); pair(z, flipped(z, range(50)), 0, 30, in1=False)                   # 50: `<=` accepts, `<` does not
    z = base(); pair(z, flipped(z, range(51)), 0, 31, in0=False, in1=False)        # 51: neither
    z = base(); pair(z, flipped(z, range(49)), 0, 32)                              # 49: both
    w = base(); add(A, w, 0.0, 40); add(B, flipped(w, range(10)), 0.0, 40); add(B, flipped(w, range(10, 20)), 0.0, 40)   # equal second
    for rot, node in ((60, 60), (60, 61), (120, 62), (120, 63)):                   # two more bins of two matches each
        v = base(); pair(v, v, rot, node)
    v = base(); pair(v, v, 180, 50, in0=False, in1=False)                          # a fourth bin with one match: rejected
    v = base(); pair(v, v, 0, 70, in1=False, pb=0)                                 # no point on side b: only mode 1 cares
    v = base(); add(A, v, 0.0, 80); add(B, v, 0.0, 81)                             # nodes not shared
    v = base(); add(A, v, 0.0, -1); add(B, v, 0.0, -1)                             # in no node

    def side(rows):
        return {"desc": np.stack([r[0] for r in rows]), "angle": np.array([r[1] for r in rows], F32),
                "node": np.array([r[2] for r in rows], np.int32), "has_point": np.array([r[3] for r in rows], np.uint8)}
    return side(A), side(B), {0: want0, 1: want1}


# ---- seeded search cases ---------------------------------------------------------------------------------------------------
FAMILY_CASES = {"nodes12": dict(seed=11, na=300, nb=300, n_nodes=12), "node1": dict(seed=12, na=300, nb=300, n_nodes=1),
                "unequal": dict(seed=13, na=240, nb=300, n_nodes=12)}
SETTINGS = [(mode, ori, ratio) for mode in (0, 1) for ori in (0, 1) for ratio in (0.7, 0.9)]


@functools.lru_cache(maxsize=None)
def family_pair(name):
    return keyframes.bow_pair(**FAMILY_CASES[name])


@functools.lru_cache(maxsize=None)
def family_reference(name, mode, ori, ratio, skip_rule=True):
    a, b = family_pair(name)
    return so.search_by_bow(a, b, mode, ratio, ori, skip_rule=skip_rule)


def empty_side():
    return {"desc": np.zeros((0, 32), np.uint8), "angle": np.zeros(0, F32), "node": np.zeros(0, np.int32), "has_point": np.zeros(0, np.uint8)}


def degenerate_pairs():
    a, b = family_pair("unequal")
    disjoint = dict(b, node=(b["node"] + 5).astype(np.int32))          # a's ids are 1000 + 37 i: no id survives + 5
    none = dict(b, node=np.full(len(b["node"]), -1, np.int32))
    return {"empty_a": (empty_side(), b), "empty_b": (a, empty_side()), "both_empty": (empty_side(), empty_side()),
            "disjoint": (a, disjoint), "no_nodes": (a, none)}


def oversized_side(n=8192):
    rng = synth.Rng(77)
    return {"desc": rng.integers(n * 32, 0, 256).astype(np.uint8).reshape(n, 32), "angle": np.zeros(n, F32),
            "node": np.zeros(n, np.int32), "has_point": np.ones(n, np.uint8)}


# ---- seeded transform cases ------------------------------------------------------------------------------------------------
TRANSFORM_CASES = {
    "full_k10_L3": dict(vocab=dict(seed=21, k=10, L=3), n=300, levelsup=(1,)),
    "pruned_k3_L6": dict(vocab=dict(seed=22, k=3, L=6, p_prune=0.25, p_stop=0.15, tie_siblings=0.3), n=200, levelsup=(0, 4, 9)),
    "wide_k20_L2": dict(vocab=dict(seed=23, k=20, L=2, p_stop=0.05), n=150, levelsup=(0, 1)),
    # 10^4 words and a frame at the documented limit of 8191 features: thousands of distinct words, 32 sorted keys per thread of bow_vector
    "limit_k10_L4": dict(vocab=dict(seed=24, k=10, L=4), n=8191, levelsup=(2,)),
}


@functools.lru_cache(maxsize=None)
def vocabulary(name):
    return bow.synthetic_vocabulary(**TRANSFORM_CASES[name]["vocab"])


@functools.lru_cache(maxsize=None)
def second_opinion_vocabulary(name):
    v = vocabulary(name)
    return so.Vocab(v["k"], v["L"], v["weighting"], v["parent"], v["desc"], v["weight"], v["is_leaf"])


def features_for(v, n, seed):
    """n descriptors: a third random, a third copies of node descriptors (distance 0 to a node - and to its twin where siblings
    are tied), a third node descriptors with a few bits flipped"""
    rng = synth.Rng(seed)
    out = rng.integers(n * 32, 0, 256).astype(np.uint8).reshape(n, 32)
    pick = rng.integers(n, 0, len(v["parent"]))
    for i in range(n):
        if i % 3 == 1:
            out[i] = v["desc"][pick[i]]
        elif i % 3 == 2:
            out[i] = synth._flip(rng, v["desc"][pick[i]], 12)
    return out


@functools.lru_cache(maxsize=None)
def transform_features(name):
    return features_for(vocabulary(name), TRANSFORM_CASES[name]["n"], 100 + len(name))


@functools.lru_cache(maxsize=None)
def transform_reference(name, levelsup):
    return second_opinion_vocabulary(name).transform(transform_features(name), levelsup)


def bow_val_bound(n):
    """|device - second opinion| <= (n + 2) 2^-52 relative: the weights are floats, so the per-word sums are exact in either
    order; the only reorderable operation is the L1 sum of at most n doubles (n - 1 roundings of 2^-53 each way), then one
    division each."""
    return (n + 2) * 2.0 ** -52
