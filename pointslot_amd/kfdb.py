"""The keyframe database on the device (ps_kfdb): KeyFrameDatabase::add / erase / clear / DetectLoopCandidates /
DetectRelocalizationCandidates of the reference (src/KeyFrameDatabase.cc:41-310) and the vocabulary score of
LoopClosing::DetectLoop's minScore loop (src/LoopClosing.cc:127-141).  A BowVector is a pair (bow_id int32 ascending, bow_val
float64), exactly what Vocabulary.transform returns; keyframes go by caller-chosen integer ids."""
import ctypes

import numpy as np

from ._lib import lib, check, PS_ERR_CAPACITY, PS_ERR_INVALID, _KfdbQueryProblem

RELOCALIZATION, LOOP = 0, 1
MAX_WORDS = 8191
MAX_CAPACITY = 4096


def _bow(bow):
    ids = np.ascontiguousarray(bow[0], np.int32).reshape(-1)
    val = np.ascontiguousarray(bow[1], np.float64).reshape(-1)
    if len(ids) != len(val):
        raise ValueError("a BowVector's ids and values differ in length")
    return ids, val


def select(mode, min_score, result, neighbours):
    """The covisibility stage (ps_kfdb_select, host only) over one query result: neighbours maps a keyframe id to the ordered
    ids of its GetBestCovisibilityKeyFrames(10) (a dict or a callable; missing = none).  Returns the candidate ids."""
    sid = np.ascontiguousarray(result["share_id"], np.int64)
    sw = np.ascontiguousarray(result["share_words"], np.int32)
    ss = np.ascontiguousarray(result["share_score"], np.float32)
    n = len(sid)
    get = neighbours if callable(neighbours) else (lambda k: neighbours.get(k, ()))
    neigh = np.zeros((max(n, 1), 10), np.int64)
    neigh_n = np.zeros(max(n, 1), np.int32)
    for i in range(n):
        if sw[i] > result["min_common_words"]:
            ids = list(get(int(sid[i])))[:10]
            neigh[i, :len(ids)] = ids
            neigh_n[i] = len(ids)
    out = np.zeros(max(n, 1), np.int64)
    nc = ctypes.c_int32(0)
    check(lib.ps_kfdb_select(int(mode), float(min_score), sid.ctypes.data, sw.ctypes.data, ss.ctypes.data, n, int(result["min_common_words"]),
                             neigh.ctypes.data, neigh_n.ctypes.data, out.ctypes.data, ctypes.byref(nc)))
    return [int(x) for x in out[:nc.value]]


class KeyFrameDatabase:
    """A mutable store of BowVectors in HBM and the place-recognition queries over it."""

    def __init__(self, capacity, max_words, device=0, matcher=None):
        self._h = ctypes.c_void_p()
        self.device = device
        self._matcher = matcher
        check(lib.ps_kfdb_create(device, int(capacity), int(max_words), ctypes.byref(self._h)))

    def _m(self):
        if self._matcher is None:
            from .matcher import ORBmatcher
            self._matcher = ORBmatcher(device=self.device)
        return self._matcher._h

    def close(self):
        if self._h:
            lib.ps_kfdb_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = ctypes.c_int32(0)
        check(lib.ps_kfdb_size(self._h, ctypes.byref(n)))
        return n.value

    def add(self, ids, bows, partial_ok=False):
        """KeyFrameDatabase::add for a batch.  Returns one bool per entry: stored, or - when partial_ok lets the call return after
        PS_ERR_CAPACITY - failed alone (longer than max_words, or no room left)."""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        n = len(ids)
        if len(bows) != n:
            raise ValueError("one BowVector per id")
        if n == 0:
            return []
        keep = [_bow(b) for b in bows]
        pid = (ctypes.c_void_p * n)(*[k[0].ctypes.data if len(k[0]) else None for k in keep])
        pval = (ctypes.c_void_p * n)(*[k[1].ctypes.data if len(k[0]) else None for k in keep])
        cnt = np.array([len(k[0]) for k in keep], np.int32)
        stored = np.zeros(n, np.int32)
        rc = lib.ps_kfdb_add(self._h, self._m(), ids.ctypes.data, pid, pval, cnt.ctypes.data, n, stored.ctypes.data)
        if not (partial_ok and rc == PS_ERR_CAPACITY):
            check(rc)
        return [bool(x) for x in stored]

    def erase(self, ids):
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        check(lib.ps_kfdb_erase(self._h, ids.ctypes.data, len(ids)))

    def clear(self):
        check(lib.ps_kfdb_clear(self._h))

    def query(self, queries, partial_ok=False):
        """queries: dicts with "bow" (a BowVector), "mode" (RELOCALIZATION or LOOP) and for LOOP "excluded", the ids of the
        connected keyframes.  Returns per query a dict: share_id int64 [nshare] in the reference's list order, share_words int32,
        share_score float32, min_common_words; "failed" = True for a query beyond the limit under partial_ok."""
        nq = len(queries)
        if nq == 0:
            return []
        room = max(len(self), 1)
        arr = (_KfdbQueryProblem * nq)()
        keep = []
        for i, q in enumerate(queries):
            ids, val = _bow(q["bow"])
            ex = np.ascontiguousarray(q.get("excluded", ()), np.int64).reshape(-1)
            o = dict(share_id=np.zeros(room, np.int64), share_words=np.zeros(room, np.int32), share_score=np.zeros(room, np.float32))
            p = arr[i]
            p.n = len(ids); p.bow_id = ids.ctypes.data if len(ids) else None; p.bow_val = val.ctypes.data if len(ids) else None
            p.mode = int(q.get("mode", RELOCALIZATION)); p.nexcluded = len(ex); p.excluded = ex.ctypes.data if len(ex) else None
            p.nshare = -2; p.min_common_words = 0
            for name, v in o.items():
                setattr(p, name, v.ctypes.data)
            keep.append((ids, val, ex, o))
        rc = lib.ps_kfdb_query(self._h, self._m(), arr, nq)
        if not (partial_ok and rc == PS_ERR_CAPACITY):
            check(rc)
        res = []
        for i, (_, _, _, o) in enumerate(keep):
            n = max(arr[i].nshare, 0)
            res.append(dict(share_id=o["share_id"][:n].copy(), share_words=o["share_words"][:n].copy(), share_score=o["share_score"][:n].copy(),
                            min_common_words=arr[i].min_common_words, failed=arr[i].nshare < 0))
        return res

    def score(self, bow, ids, unknown_ok=False):
        """L1Scoring::score(bow, stored keyframe) in double for the named keyframes; NaN for an id that is not stored (an error
        unless unknown_ok)."""
        qi, qv = _bow(bow)
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        out = np.zeros(max(len(ids), 1), np.float64)
        rc = lib.ps_kfdb_score(self._h, self._m(), qi.ctypes.data if len(qi) else None, qv.ctypes.data if len(qi) else None, len(qi),
                               ids.ctypes.data, len(ids), out.ctypes.data)
        if not (unknown_ok and rc == PS_ERR_INVALID and len(ids) and np.isnan(out[:len(ids)]).any()):
            check(rc)
        return out[:len(ids)]

    def detect_loop_candidates(self, bow, connected_ids, min_score, neighbours):
        """DetectLoopCandidates(pKF, minScore): connected_ids = pKF->GetConnectedKeyFrames()"""
        r = self.query([dict(bow=bow, mode=LOOP, excluded=connected_ids)])[0]
        return select(LOOP, min_score, r, neighbours)

    def detect_relocalization_candidates(self, bow, neighbours):
        """DetectRelocalizationCandidates(F)"""
        r = self.query([dict(bow=bow, mode=RELOCALIZATION)])[0]
        return select(RELOCALIZATION, 0.0, r, neighbours)
