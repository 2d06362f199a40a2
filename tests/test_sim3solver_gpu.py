"""ps_sim3_ransac and pointslot_amd.Sim3Solver on the device against the restatement (tests/sim3solver_second_opinion.py) over the
seeded cases of tests/sim3solver_cases.py.

The check stage is exact arithmetic given the model: the device's mask must equal, bit for bit, the restatement's CheckInliers applied
to the device's own float32 model, and the count its popcount - no tolerance.  The model is the rounding of FP64 values: it must equal
the restatement's bit for bit, except on at most 1 % of the hypotheses of a case, where every entry is within one float32 ulp.  That cap
is a condition, not a measurement: tests/test_sim3solver_cpu.py shows that the restatement's two eigen solvers never differ on these
inputs.  Degenerate cases (a zero imaginary part, a near-collinear triple) are compared on counts only."""
import hashlib
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import sim3solver_cases as sc
import sim3solver_second_opinion as so

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(sc.CASES)


@pytest.fixture(scope="module")
def matcher():
    from pointslot_amd.matcher import ORBmatcher
    m = ORBmatcher()
    yield m
    m.close()


_DEVICE = {}


def device(matcher, name):
    """the device's run of one case alone, computed once and shared: treat as read-only"""
    if name not in _DEVICE:
        from pointslot_amd.sim3solver import sim3_ransac
        _DEVICE[name] = sim3_ransac(matcher, [sc.problem(sc.CASES[name])])[0]
    return _DEVICE[name]


def _served(case):
    return case["n"] >= case["min_inliers"] and case["n"] >= 3 and len(case["draws"]) > 0


def _popcount(words):
    return sum(bin(int(w)).count("1") for w in words)


def _ulps(a, b):
    """distance in float32 ulps per entry (NaN against NaN: 0)"""
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    both_nan = np.isnan(a) & np.isnan(b)
    return np.where(both_nan, 0, np.where(np.isnan(a) | np.isnan(b), 1 << 40, d))


@pytest.mark.parametrize("name", NAMES)
def test_mask_and_count_are_exact_given_the_model(matcher, name):
    c, d = sc.CASES[name], device(matcher, name)
    if not _served(c):
        assert len(d["inliers"]) == 0 and d["first_success"] == -1 and d["best"] == -1
        return
    nhyp = len(c["draws"])
    assert d["inliers"].shape == (nhyp,) and d["model"].shape == (nhyp, 13) and d["mask"].shape == (nhyp, (c["n"] + 63) // 64)
    for h in range(nhyp):
        sR12, t12, sR21, t21 = so.pair_from_model13(d["model"][h])
        inl = so.check_inliers(c["x3dc1"], c["x3dc2"], c["max_err1"], c["max_err2"], c["k1"], c["k2"], sR12, t12, sR21, t21)
        assert np.array_equal(d["mask"][h], so.mask_words(inl)), (name, h)
        assert int(d["inliers"][h]) == _popcount(d["mask"][h]) == int(inl.sum()), (name, h)
        if np.isnan(d["model"][h]).any():
            assert d["inliers"][h] == 0


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_restatement(matcher, name):
    c, d = sc.CASES[name], device(matcher, name)
    if not _served(c):
        return
    e = sc.expected(name)
    if c["degenerate"]:
        if name == "pure_translation":
            assert np.isnan(d["model"][:, 1:10]).all() and (d["inliers"] == 0).all()       # the reference's 0 * (1 / 0)
            assert np.array_equal(d["inliers"], e["inliers"])
        else:                                                                              # the hypotheses with an eigenvalue gap
            ok = e["gap"] >= 1e-6
            assert ok.sum() >= len(ok) - 4
            assert np.array_equal(d["inliers"][ok], e["inliers"][ok])
        return
    same = (d["model"].view(np.uint32) == e["model"].view(np.uint32)).all(1)
    print("%s: %d of %d models bit-equal" % (name, same.sum(), len(same)))
    assert (~same).sum() <= len(same) // 100, (name, np.nonzero(~same)[0])
    assert _ulps(d["model"], e["model"]).max() <= 1
    assert np.array_equal(d["mask"][same], e["mask"][same]) and np.array_equal(d["inliers"][same], e["inliers"][same])


class _Fed(so.Sim3SolverRef):
    """the restatement's sequential loop fed with recorded per-hypothesis results"""

    def evaluate(self, idx):
        h = self.mnIterations - 1
        assert idx == so.draw_triple_list(self.fed_draws[h], self.N)
        words = self.fed["mask"][h]
        inl = np.array([(int(words[i >> 6]) >> (i & 63)) & 1 for i in range(self.N)], bool)
        return self.fed["model"][h], inl, int(self.fed["inliers"][h])


def _t12(m13):
    sR12, t12, _, _ = so.pair_from_model13(m13)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = sR12; T[:3, 3] = t12
    return T


@pytest.mark.parametrize("name", NAMES)
def test_sequence_outcome(matcher, name):
    from pointslot_amd.sim3solver import Sim3Solver
    c, d = sc.CASES[name], device(matcher, name)
    n = c["n"]
    if _served(c):
        assert (d["first_success"], d["best"]) == so.sequence_outcome(d["inliers"], c["min_inliers"])
    # the class: the whole iterate(5) sequence against the restatement's loop fed with the device's counts
    idx1, n1 = 2 * np.arange(n) + 1, 2 * n + 3
    args = (c["x3dc1"], c["x3dc2"], c["max_err1"], c["max_err2"], c["k1"], c["k2"], c["fix_scale"])
    flat = [int(v) for v in c["draws"].reshape(-1)]
    S = Sim3Solver.from_arrays(*args, indices1=idx1, n1=n1, matcher=matcher, rand=itertools.cycle(flat).__next__)
    S.SetRansacParameters(0.99, c["min_inliers"], 300)
    ref = _Fed.from_arrays(*args, rand=itertools.cycle(flat).__next__, indices1=idx1, n1=n1)
    ref.SetRansacParameters(0.99, c["min_inliers"], 300)
    assert S.mRansacMaxIts == ref.mRansacMaxIts and S.N == ref.N
    its = ref.mRansacMaxIts
    whole = its <= len(c["draws"])                       # the class's hypotheses are the case's first `its`
    if _served(c):
        if whole:
            ref.fed, ref.fed_draws = d, c["draws"]
        else:                                            # the draws wrap around: the class's own run is the record
            Sim3Solver.PrepareBatch([S])
            ref.fed, ref.fed_draws = S._res, np.array([flat[k % len(flat)] for k in range(3 * its)]).reshape(-1, 3)
    own = None
    if _served(c) and whole and not c["degenerate"]:
        e = sc.expected(name)
        first = so.sequence_outcome(e["inliers"][:its], c["min_inliers"])[0]
        upto = its if first < 0 else first + 1
        if np.array_equal(d["model"][:upto].view(np.uint32), e["model"][:upto].view(np.uint32)):
            own = _Fed.from_arrays(*args, rand=itertools.cycle(flat).__next__, indices1=idx1, n1=n1)   # the restatement's own run
            own.SetRansacParameters(0.99, c["min_inliers"], 300)
            own.fed, own.fed_draws = e, c["draws"]
    nfound = 0
    for call in range(its + 3):                          # (a call that returns a model ends early: up to `its` calls)
        T, noMore, vb, nIn = S.iterate(5)
        for r in (ref, own):
            if r is None:
                continue
            m, noMore_r, vb_r, nIn_r = r.iterate(5)
            assert (T is None) == (m is None) and bool(noMore) == bool(noMore_r) and nIn == nIn_r, (name, call)
            assert vb.shape == (n1,) and np.array_equal(vb, vb_r), (name, call)
            assert S.mnIterations == r.mnIterations and S.mnBestInliers == r.mnBestInliers
            if m is not None:
                assert np.array_equal(T.view(np.uint32), _t12(m).view(np.uint32))
                assert np.array_equal(S.GetEstimatedRotation(), m[1:10].reshape(3, 3)) and S.GetEstimatedScale() == m[0]
                assert not vb[::2].any() and vb.sum() == nIn                       # only the slots of mvnIndices1
        nfound += T is not None
        if T is not None:
            own = None                                   # (outright only up to the first success)
        if noMore:
            break
    assert noMore
    assert S.mnIterations == (its if _served(c) else 0)
    if name in sc.SOLVABLE:
        assert nfound >= 1
    if name in ("no_success", "n_eq_min", "n_lt_min", "pure_translation"):
        assert nfound == 0


def _digest(results):
    h = hashlib.sha256()
    for r in results:
        for k in ("inliers", "model", "mask"):
            h.update(np.ascontiguousarray(r[k]).tobytes())
        h.update(np.array([r["first_success"], r["best"]], np.int32).tobytes())
    return h.hexdigest()


def test_ragged_batch_equals_one_by_one_and_ignores_old_memory(matcher):
    from pointslot_amd import _lib
    from pointslot_amd.sim3solver import sim3_ransac
    probs = [sc.problem(sc.CASES[k]) for k in sc.RAGGED]
    batch = sim3_ransac(matcher, probs)
    ms = matcher.last_kernel_ms()
    assert ms > 0
    for name, b in zip(sc.RAGGED, batch):
        one = device(matcher, name)
        for k in ("inliers", "model", "mask"):
            assert np.array_equal(b[k].view(np.uint8), one[k].view(np.uint8)), (name, k)
        assert (b["first_success"], b["best"]) == (one["first_success"], one["best"])
    assert len(batch[sc.RAGGED.index("n_lt_min")]["inliers"]) == 0
    without = sim3_ransac(matcher, probs, want_mask=False)                      # mask = NULL
    assert all(np.array_equal(a["inliers"], b["inliers"]) and "mask" not in a for a, b in zip(without, batch))
    _lib.poison_lds()
    assert _digest(sim3_ransac(matcher, probs)) == _digest(batch)
    # ... and in a fresh process whose new device buffers are filled with 0xFF bytes
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import sim3solver_cases as sc, test_sim3solver_gpu as t\n"
            "from pointslot_amd.matcher import ORBmatcher\n"
            "from pointslot_amd.sim3solver import sim3_ransac\n"
            "print('digest', t._digest(sim3_ransac(ORBmatcher(), [sc.problem(sc.CASES[k]) for k in sc.RAGGED])))\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, PS_DEBUG_FILL="255"), timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "digest " + _digest(batch)


def test_an_oversize_problem_fails_alone(matcher):
    from pointslot_amd import _lib
    from pointslot_amd.sim3solver import sim3_ransac
    big = dict(sc.problem(sc.CASES["n21"]))
    n = 32768
    big.update(x3dc1=np.tile(np.float32([0, 0, 5]), (n, 1)), x3dc2=np.tile(np.float32([0, 0, 5]), (n, 1)), max_err1=np.ones(n, np.float32),
               max_err2=np.ones(n, np.float32), draws=big["draws"][:4])
    many = dict(sc.problem(sc.CASES["n21"]))
    many["draws"] = np.zeros((4097, 3), np.int32)
    probs = [sc.problem(sc.CASES["n64"]), big, sc.problem(sc.CASES["n65_fix"]), many]
    with pytest.raises(_lib.PointslotError) as err:
        sim3_ransac(matcher, probs)
    assert err.value.code == _lib.PS_ERR_CAPACITY
    res = sim3_ransac(matcher, probs, partial_ok=True)
    assert res[1]["first_success"] == -2 and res[1]["best"] == -2 and len(res[1]["inliers"]) == 0
    assert res[3]["first_success"] == -2 and len(res[3]["inliers"]) == 0
    for k, name in ((0, "n64"), (2, "n65_fix")):
        one = device(matcher, name)
        assert np.array_equal(res[k]["inliers"], one["inliers"]) and np.array_equal(res[k]["mask"], one["mask"])
        assert np.array_equal(res[k]["model"].view(np.uint32), one["model"].view(np.uint32))
        assert res[k]["first_success"] == one["first_success"]
    # at the limits the call is served
    edge = dict(big)
    edge.update({k: big[k][:32767] for k in ("x3dc1", "x3dc2", "max_err1", "max_err2")})
    r = sim3_ransac(matcher, [edge])[0]
    assert r["inliers"].shape == (4,) and r["mask"].shape == (4, 512)
