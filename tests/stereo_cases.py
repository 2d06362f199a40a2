"""The scenes of the randomised sweep over the stereo matcher (tools/stress_stereo.py: Frame::ComputeStereoMatches on two handles, on a
batch, and Frame::ComputeObjStereoMatches on caller key sets) and of tests/test_stereo_cases_cpu.py: scenes(seed, budget) is a
deterministic list, the first budget // 2 of them IMAGE scenes (synth.stereo_pair images of a drawn size, level count, scale factor
and quota; the keypoints are the extractor's; scene 0 is one batch of ten pairs), the others KEY-SET scenes (a small pair on the two
handles, key sets built by hand: keys on the image borders, on rows around the multiples of 8, in every octave; every right key a copy
of a left key moved by the scene's disparity, by nothing, by a few pixels or by anything in [-3, maxD + 3], its row moved to and just
past the edge of the +-2 * scale band, its octave changed by up to two, exactly k bits of its descriptor flipped with k around the
thresholds 75 and 100; groups of right keys at the same distance from one left key; the right set shuffled).  mb and mbf put
maxD = mbf / mb below one pixel, at a few pixels, around the scene's disparities and beyond the image width.  Pure numpy on
pointslot_amd.synth's generator, the oracle and the second opinion; no GPU code.  Test infrastructure.

gate_counts(scene) runs orb_second_opinion.stereo_matches with its counters (no copy of the function) on the padded planes.  Under
the committed seed and budget, sweep_cases.COMMITTED["stereo"] = (20250605, 26) - 13 image scenes with 22 pairs, 13 key-set scenes -
the left keypoints of the run leave the loop as follows (tests/test_stereo_cases_cpu.py asserts the lower bounds of the issue):

    empty_row 387, hamming 4977, endu 236, sad_edge 479, negative 806, beyond_max_d 328, zero_clamp 88, median_cut 1664, tie 458,
    win_74 273, loss_75 191, accepted 4461

(empty_row: no right keypoint on the row; hamming: best distance >= 75; endu: `endu >= cols`; sad_edge: SAD minimum at shift +-5;
negative / beyond_max_d: disparity < 0 / >= maxD; zero_clamp: the `disparity <= 0` clamp; median_cut: removed by the median cut; tie:
two or more candidates at the winning distance; win_74 / loss_75: best distance exactly 74 / 75.)  Two scenes end with exactly 1 and 2
accepted matches, the pairs with the left image on both sides end with median SAD 0 and nothing kept, and both entries see an empty
right set beside a non-empty left one.

Four exits cannot be reached with keys inside the image and are not chased: `maxU < 0` and `iniu < 0` need x < 0; `|deltaR| > 1` and a
NaN parabola cannot arise, because the minimum is the FIRST smallest SAD and not at +-5, so d1 > d2 <= d3, which makes
|deltaR| <= 0.5 and the denominator positive."""
import functools
import math

import numpy as np

import oracle_lib
import orb_second_opinion as so
import sweep_cases
from pointslot_amd import synth

F32 = np.float32
LEVELS = (1, 3, 5, 8)
SCALES = (1.1, 1.2, 1.4, 2.0)
NFEATURES = (200, 1000, 2000)
N_LEFT = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1000, 4096)
N_RIGHT = (0, 1, 7, 300, 4096)
FLIPS = (0, 10, 40, 73, 74, 75, 76, 99, 100, 101)
_FLIP_SHARE = (0.3, 0.15, 0.1, 0.05, 0.1, 0.1, 0.05, 0.05, 0.05, 0.05)
MAXD_KINDS = ("below_one", "few", "scene", "wide")
BFS = (60.0, 120.0, 200.0)               # the right image is the left warped by bf / z(y), z = 60 (top) .. 6 (bottom): up to 10, 20, 33 px
INI_TH, MIN_TH = 20, 5
MAX_WIDTH = 640
BATCH_KINDS = ("stereo", "stereo", "same", "stereo", "right_blank", "blank", "stereo", "same", "stereo", "stereo")
# the right sizes that go with N_LEFT, scene by scene (a tiny right set leaves most rows without a candidate)
_KEY_SIZES = ((1, 1), (2, 7), (3, 7), (4, 1), (5, 0), (15, 300), (16, 7), (17, 300), (63, 300), (64, 4096), (65, 300), (1000, 300), (4096, 4096))
# ... and their pyramids: the octave gate needs levels, and the large sets have them
_KEY_LEVELS = ((8, 1.2), (3, 1.4), (1, 2.0), (1, 1.4), (3, 2.0), (3, 1.2), (1, 1.1), (5, 1.1), (5, 1.4), (3, 1.1), (8, 1.2), (8, 1.1), (5, 1.2))
GATES = ("empty_row", "hamming", "endu", "sad_edge", "negative", "beyond_max_d", "zero_clamp", "median_cut", "tie", "win_74", "loss_75", "accepted")


def min_side(levels, scale):
    """the extractor's own limit (tools/stress_orb.py): the top level still holds a 30-pixel cell inside its borders"""
    return int(math.ceil(70 * scale ** (levels - 1))) + 8


def _levels_and_scale(d, limit, forced=None):
    levels, scale = forced or (d.pick(LEVELS), d.pick(SCALES))
    if scale == 2.0:
        levels = min(levels, 3)                                  # at most 4 levels at 2.0: of the draw's counts, 1 and 3
    while min_side(levels, scale) > limit:
        levels = LEVELS[LEVELS.index(levels) - 1]
    return levels, scale


def _max_d(kind, bf, w):
    return dict(below_one=0.5, few=4.0, scene=1.25 * bf / 6.0, wide=w + 50.0)[kind]


def _pair(kind, seed, w, h, bf):
    left, right = synth.stereo_pair(seed, w, h, n_rect=int(w * h / 1200), bf=bf)
    blank = np.full((h, w), 90, np.uint8)
    return dict(stereo=(left, right), same=(left, left), blank=(blank, blank), right_blank=(left, blank))[kind]


def _image_scene(d, i):
    if i == 0:      # the batch: ten pairs of one size in one call - the second grid row of st_match serves pairs 8 and 9
        levels, scale, nfeatures = 3, 1.2, 1000
        w, h = d.int(200, 300), d.int(120, 180)
        kinds, maxd_kind = BATCH_KINDS, "scene"
    else:
        forced = ((1, 2.0), (3, 1.4), (5, 1.2), (8, 1.1))[i - 1] if i <= 4 else None
        levels, scale = _levels_and_scale(d, 400, forced)
        nfeatures = d.pick(NFEATURES)
        lo = max(min_side(levels, scale), 96)
        h = d.int(lo, lo + 100)
        w = d.int(max(h, 160), MAX_WIDTH)
        kinds = (("same",), ("blank",), ("right_blank",))[i - 5] if 5 <= i <= 7 else (d.pick(("stereo", "stereo", "stereo", "same")),)
        maxd_kind = MAXD_KINDS[i % 4]
    bf = d.pick(BFS)
    mbf = F32(bf)
    mb = F32(mbf / F32(_max_d(maxd_kind, bf, w)))
    return dict(kind="image", levels=levels, scale=scale, nfeatures=nfeatures, w=w, h=h, bf=bf, maxd_kind=maxd_kind, mb=float(mb), mbf=float(mbf),
                pair_kinds=tuple(kinds), pairs=[_pair(k, d.seed(), w, h, bf) for k in kinds])


# ---- key sets built by hand --------------------------------------------------------------------------------------------------------
def _symmetric_pixels(img):
    """pixels (x, y) of an image whose 11 x 11 patch differs from the patches one column to the left and to the right by the same
    SAD > 0: matched against itself at level 0, the parabola's vertex is at 0 and the disparity comes out as exactly 0"""
    I = img.astype(np.int32)
    h, w = I.shape
    x0, x1, y0, y1 = 6, w - 12, 5, h - 5                  # (the window test needs x + 11 < w)
    if x1 <= x0 or y1 <= y0:
        return np.zeros((0, 2), np.int64)
    c = lambda s: I[y0:y1, x0 + s:x1 + s]
    d1, d3 = np.zeros((y1 - y0, x1 - x0), np.int64), np.zeros((y1 - y0, x1 - x0), np.int64)
    for dy in range(-5, 6):
        for dx in range(-5, 6):
            p = lambda s: I[y0 + dy:y1 + dy, x0 + dx + s:x1 + dx + s] - c(s)
            d1 += np.abs(p(0) - p(-1)); d3 += np.abs(p(0) - p(1))
    ys, xs = np.nonzero((d1 == d3) & (d1 > 0))
    return np.stack([xs + x0, ys + y0], 1)


def _flipped(rng, desc, k):
    """desc [n, 32] with exactly k[i] bits of row i flipped"""
    n = len(desc)
    rank = np.argsort(rng.uniform(n * 256).reshape(n, 256), axis=1, kind="stable")          # a random order of the 256 bits
    bits = np.zeros((n, 256), np.uint8)
    np.put_along_axis(bits, rank, (np.arange(256)[None, :] < np.asarray(k)[:, None]).astype(np.uint8), axis=1)
    return desc ^ np.packbits(bits, axis=1)


def _keypoints(x, y, octave, sf):
    k = np.zeros(len(x), oracle_lib.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = x, y, octave
    k["size"], k["response"], k["class_id"] = F32(31) * sf[octave], 1.0, -1
    return k


def _inside(v, n):
    return np.clip(v.astype(F32), F32(0), np.nextafter(F32(n), F32(0)))


def _key_sets(seed, w, h, sf, n_left, n_right, max_d, bf, tiny, symmetric):
    """bf: the pair's disparity is bf / z(y) (0: the left image on both handles).  tiny: the left keys lie away from the borders in
    the two lowest octaves and the first copy of each is its true match.  symmetric: pixels of _symmetric_pixels, for a quarter of
    the left keys, each with an exact copy in the right set."""
    rng = synth.Rng(seed, lanes=4096)
    U = rng.uniform
    nl = len(sf)
    # -- the left keys
    where = U(n_left)
    x, y = U(n_left) * w, U(n_left) * h
    x = np.where(where < 0.15, U(n_left) * 12, x)                                             # within 12 px of the left border
    x = np.where((where >= 0.15) & (where < 0.30), w - U(n_left) * 14, x)                     # within 14 px of the right border
    edge_y = np.where(U(n_left) < 0.5, U(n_left) * 6, h - U(n_left) * 6)                      # within 6 rows of the top or bottom
    y = np.where((where >= 0.30) & (where < 0.45), edge_y, y)
    row8 = 8 * rng.integers(n_left, 0, h // 8 + 1) + np.where(U(n_left) < 0.5, -1, 1) + U(n_left) * 0.99
    y = np.where((where >= 0.45) & (where < 0.60), row8, y)                                   # rows that are multiples of 8 +- 1
    octave = rng.integers(n_left, 0, nl)
    if tiny:
        x, y = (0.3 + 0.5 * U(n_left)) * w, (0.25 + 0.5 * U(n_left)) * h
        octave = np.minimum(octave % 2, nl - 1)
    whole = U(n_left) < 0.4
    x, y = np.where(whole, np.floor(x), x), np.where(whole, np.floor(y), y)
    exact = np.zeros(n_left, bool)
    if len(symmetric) and not tiny:
        exact = U(n_left) < 0.25
        px = symmetric[rng.integers(n_left, 0, len(symmetric))]
        x, y, octave = np.where(exact, px[:, 0], x), np.where(exact, px[:, 1], y), np.where(exact, 0, octave)
    x, y = _inside(x, w), _inside(y, h)
    desc_l = rng.integers(n_left * 32, 0, 256).astype(np.uint8).reshape(n_left, 32)
    true_d = (bf / (60.0 - 54.0 * y.astype(np.float64) / (h - 1))) if bf else np.zeros(n_left)
    # -- the right keys: groups at one descriptor distance from one left key first, then single copies, every left key in turn
    n_groups = min(n_left // 6, n_right // 8)
    src, dx, dy_mode, doct, flips = [], [], [], [], []
    for g in range(n_groups):
        s, size, k = int(rng.integers(1, 0, n_left)[0]), int(rng.integers(1, 2, 5)[0]), (0, 10, 40, 73, 74)[int(rng.integers(1, 0, 5)[0])]
        first = int(rng.integers(1, 0, size)[0])
        for j in range(size):                                     # 12 level pixels apart: more than the SAD slide can make up for
            src.append(s); dx.append(true_d[s] + (j - first) * 12.0 * float(sf[octave[s]])); dy_mode.append(0); doct.append(0); flips.append(k)
    m = n_right - len(src)
    turn = np.argsort(U(n_left), kind="stable")
    s1 = turn[np.arange(m) % n_left]
    u = U(m)
    few = U(m) * 4
    few = np.where(U(m) < 0.4, np.floor(few), few)
    anywhere = -3 + U(m) * (min(max_d, w) + 6)                    # [-3, maxD + 3], or the image's width where maxD is beyond it
    dx1 = np.where(u < 0.40, true_d[s1], np.where(u < 0.55, 0.0, np.where(u < 0.75, few, anywhere)))
    u = U(m)
    dy1 = np.where(u < 0.6, 0, np.where(u < 0.8, 1, 2)) * np.where(U(m) < 0.5, -1, 1)       # 0, +-1: on the band's edge, +-2: 1.01 past it
    u = U(m)
    do1 = np.where(u < 0.6, 0, np.where(u < 0.75, 1, np.where(u < 0.9, -1, np.where(u < 0.95, 2, -2))))
    fl1 = np.asarray(FLIPS)[np.searchsorted(np.cumsum(_FLIP_SHARE), U(m) * (1 - 1e-9))]
    first_copy = np.arange(m) < n_left
    own = first_copy & (exact[s1] | tiny)                         # the copy that is the true match
    dx1 = np.where(own, true_d[s1], dx1); dy1 = np.where(own, 0, dy1); do1 = np.where(own, 0, do1); fl1 = np.where(own, 0, fl1)
    src = np.concatenate([np.asarray(src, np.int64), s1]).astype(np.int64)
    dx = np.concatenate([np.asarray(dx, np.float64), dx1]); dy_mode = np.concatenate([np.asarray(dy_mode, np.int64), dy1])
    doct = np.concatenate([np.asarray(doct, np.int64), do1]); flips = np.concatenate([np.asarray(flips, np.int64), fl1])
    oct_r = np.clip(octave[src] + doct, 0, nl - 1)
    band = F32(2.0) * sf[oct_r]                                                              # the reference's r = 2 * mvScaleFactors[octave]
    step = np.where(np.abs(dy_mode) == 2, band + F32(1.01), np.where(dy_mode == 0, F32(0), band)).astype(F32)
    xr = _inside(x[src] - dx.astype(F32), w)
    yr = _inside(y[src] + np.sign(dy_mode).astype(F32) * step, h)
    desc_r = _flipped(rng, desc_l[src], flips)
    order = np.argsort(U(n_right), kind="stable")                 # "the first smallest wins" is decided by the index
    kl, kr = _keypoints(x, y, octave, sf), _keypoints(xr[order], yr[order], oct_r[order], sf)
    return kl, desc_l, kr, np.ascontiguousarray(desc_r[order]), dict(src=src[order], flips=flips[order], exact=exact)


def _key_scene(d, i):
    n_left, n_right = _KEY_SIZES[i] if i < len(_KEY_SIZES) else (d.pick(N_LEFT), d.pick(N_RIGHT))
    levels, scale = _levels_and_scale(d, 280, _KEY_LEVELS[i] if i < len(_KEY_LEVELS) else None)
    nfeatures = d.pick(NFEATURES)
    lo = max(min_side(levels, scale), 96)
    h = d.int(lo, lo + 40)
    w = d.int(max(h, 160), max(h, 160) + 160)
    tiny = n_left <= 5
    kind = "same" if i % 3 == 2 else "stereo"
    maxd_kind = "scene" if tiny else MAXD_KINDS[(i + 2) % 4]
    bf = d.pick(BFS)
    max_d = _max_d(maxd_kind, bf, w)
    mbf = F32(bf)
    mb = F32(mbf / F32(max_d))
    left, right = _pair(kind, d.seed(), w, h, bf)
    sf, _ = so.scale_tables(levels, scale)
    kl, dl, kr, dr, made = _key_sets(d.seed(), w, h, sf, n_left, n_right, max_d, 0.0 if kind == "same" else bf, tiny,
                                     _symmetric_pixels(left) if kind == "same" else ())
    return dict(kind="keys", levels=levels, scale=scale, nfeatures=nfeatures, w=w, h=h, bf=bf, maxd_kind=maxd_kind, mb=float(mb), mbf=float(mbf),
                pair_kinds=(kind,), pairs=[(left, right)], kps_l=kl, desc_l=dl, kps_r=kr, desc_r=dr, made=made)


@functools.lru_cache(maxsize=None)
def scenes(seed, budget):
    """budget // 2 image scenes (the first is the batch), then the key-set scenes.  The arrays are shared: do not write into them."""
    d = sweep_cases._Draw(int(seed))
    n_img = int(budget) // 2
    return [_image_scene(d, i) for i in range(n_img)] + [_key_scene(d, i) for i in range(int(budget) - n_img)]


# ---- the references ------------------------------------------------------------------------------------------------------------------
def extracted(scene, pair):
    """the oracle's two extractors after they have run on the pair, with their keypoints and descriptors"""
    ol, orr = (oracle_lib.OracleORB(scene["nfeatures"], scene["scale"], scene["levels"], INI_TH, MIN_TH) for _ in range(2))
    left, right = scene["pairs"][pair]
    kl, dl = ol.run(left)
    kr, dr = orr.run(right)
    return ol, orr, kl, dl, kr, dr


def _key_sets_of(scene, ex):
    if scene["kind"] == "keys":
        return scene["kps_l"], scene["desc_l"], scene["kps_r"], scene["desc_r"]
    return ex[2:]


def oracle_of(scene):
    """(kept, uRight, depth) per pair: oracle_lib.stereo_match for an image scene, stereo_match_keys for a key-set scene"""
    out = []
    for p in range(len(scene["pairs"])):
        ex = extracted(scene, p)
        if scene["kind"] == "keys":
            out.append(oracle_lib.stereo_match_keys(ex[0], ex[1], *_key_sets_of(scene, ex), scene["mb"], scene["mbf"]))
        else:
            out.append(oracle_lib.stereo_match(ex[0], ex[1], scene["mb"], scene["mbf"]))
    return out


def gate_counts(scene):
    """per pair: (kept, uRight, depth, counts) of orb_second_opinion.stereo_matches on the padded planes - counts: how often each exit
    of the loop was taken (GATES; "tie": left keys with two or more candidates at the winning distance, "win_74" / "loss_75": best
    distance exactly 74 / 75), the accepted matches and, where there are any, the median SAD; n_left and n_right beside them"""
    out = []
    sf, isf = so.scale_tables(scene["levels"], scene["scale"])
    for p in range(len(scene["pairs"])):
        ex = extracted(scene, p)
        kl, dl, kr, dr = _key_sets_of(scene, ex)
        planes = [[e.padded(l) for l in range(scene["levels"])] for e in ex[:2]]
        counts = {g: 0 for g in GATES}
        kept, ur, dp = so.stereo_matches(kl, dl, kr, dr, planes[0], planes[1], sf, isf, F32(scene["mb"]), F32(scene["mbf"]), border=so.EDGE, counts=counts)
        counts["n_left"], counts["n_right"] = len(kl), len(kr)
        out.append((kept, ur, dp, counts))
    return out


def counts_line(totals):
    """the totals of a run as the module's docstring states them"""
    return ", ".join("%s %d" % (g, totals[g]) for g in GATES)


@functools.lru_cache(maxsize=None)
def references(seed, budget):
    """(oracle_of, gate_counts) of every scene, computed once per process"""
    return [(oracle_of(s), gate_counts(s)) for s in scenes(seed, budget)]
