"""The DBoW2 vocabulary on the device (ps_vocabulary, ps_bow_transform): ORBVocabulary's loadFromBinaryFile and
transform(features, BowVector, FeatureVector, levelsup) - /root/reference/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1343-1384,
:1133-1200 - which Frame::ComputeBoW and KeyFrame::ComputeBoW call (src/Frame.cc:2040-2047, src/KeyFrame.cc:114-123).  Also the
writer of the binary layout and a seeded tree generator: training a vocabulary is out of scope, and ORBvoc.bin is not in the tree."""
import ctypes
import struct

import numpy as np

from . import synth
from ._lib import lib, check

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM = 0
MAX_N = 8191


class _BowProblem(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("desc", ctypes.c_void_p), ("levelsup", ctypes.c_int32), ("word", ctypes.c_void_p),
                ("node", ctypes.c_void_p), ("bow_id", ctypes.c_void_p), ("bow_val", ctypes.c_void_p), ("bow_n", ctypes.c_int32)]


lib.ps_vocabulary_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
lib.ps_vocabulary_load_binary.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
lib.ps_vocabulary_destroy.argtypes = [ctypes.c_void_p]
lib.ps_vocabulary_destroy.restype = None
lib.ps_vocabulary_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int32)] * 4
lib.ps_bow_transform.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_BowProblem), ctypes.c_int]


def save_binary(path, k, L, weighting, parent, desc, weight, is_leaf, scoring=L1_NORM):
    """The layout loadFromBinaryFile reads: u32 nb_nodes, u32 size_node = 41, i32 k, L, scoring, weighting, then per record
    i32 parent, 32 B descriptor, f32 weight, u8 leaf."""
    n = len(parent)
    rec = np.zeros(n, np.dtype([("parent", "<i4"), ("desc", "u1", 32), ("weight", "<f4"), ("leaf", "u1")]))
    assert rec.dtype.itemsize == 41
    rec["parent"] = np.asarray(parent, np.int32)
    rec["desc"] = np.asarray(desc, np.uint8).reshape(n, 32)
    rec["weight"] = np.asarray(weight, np.float32)
    rec["leaf"] = (np.asarray(is_leaf) != 0).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(struct.pack("<IIiiii", n, 41, int(k), int(L), int(scoring), int(weighting)))
        f.write(rec.tobytes())


class Vocabulary:
    """An immutable vocabulary tree in HBM.  Any number of matchers may read it."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = device
        self._matcher = None

    @classmethod
    def from_arrays(cls, k, L, weighting, parent, desc, weight, is_leaf, scoring=L1_NORM, device=0, depth=None):
        """records in file order: record i becomes node i + 1 (root = 0), children in record order, word ids in leaf order
        (depth: what synthetic_vocabulary adds for its users; not part of a vocabulary)"""
        parent = np.ascontiguousarray(parent, np.int32)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        weight = np.ascontiguousarray(weight, np.float32)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        n = len(parent)
        if not (len(desc) == len(weight) == len(is_leaf) == n):
            raise ValueError("the record arrays differ in length")
        h = ctypes.c_void_p()
        check(lib.ps_vocabulary_create(device, int(k), int(L), int(scoring), int(weighting), n, parent.ctypes.data, desc.ctypes.data,
                                       weight.ctypes.data, is_leaf.ctypes.data, ctypes.byref(h)))
        return cls(h, device)

    @classmethod
    def load(cls, path, device=0):
        """ORBVocabulary::loadFromBinaryFile"""
        h = ctypes.c_void_p()
        check(lib.ps_vocabulary_load_binary(device, str(path).encode(), ctypes.byref(h)))
        return cls(h, device)

    save_binary = staticmethod(save_binary)

    def info(self):
        v = [ctypes.c_int32(0) for _ in range(4)]
        check(lib.ps_vocabulary_info(self._h, *[ctypes.byref(x) for x in v]))
        return dict(k=v[0].value, L=v[1].value, nodes=v[2].value, words=v[3].value)

    def size(self):
        return self.info()["words"]

    def close(self):
        if self._h:
            lib.ps_vocabulary_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transform(self, descriptors, levelsup=4, matcher=None, partial_ok=False):
        """transform(features, BowVector, FeatureVector, levelsup) for a batch of frames.  descriptors: one uint8 [n, 32] array
        per frame; levelsup: one value or one per frame.  Returns per frame a dict: word int32 [n], node int32 [n] (-1: stopped),
        bow_id int32 [m] ascending, bow_val float64 [m]; "failed" = True for a frame beyond the limit when partial_ok lets the
        call return after PS_ERR_CAPACITY.  The FeatureVector is node -> features in ascending order (feature_vector)."""
        if matcher is None:
            if self._matcher is None:
                from .matcher import ORBmatcher
                self._matcher = ORBmatcher(device=self.device)
            matcher = self._matcher
        nf = len(descriptors)
        lv = [int(levelsup)] * nf if np.ndim(levelsup) == 0 else [int(x) for x in levelsup]
        arr = (_BowProblem * max(nf, 1))()
        keep = []
        for i, d in enumerate(descriptors):
            d = np.ascontiguousarray(d, np.uint8).reshape(-1, 32)
            n = len(d)
            o = dict(word=np.full(max(n, 1), -2, np.int32), node=np.full(max(n, 1), -2, np.int32), bow_id=np.zeros(max(n, 1), np.int32),
                     bow_val=np.zeros(max(n, 1), np.float64))
            p = arr[i]
            p.n = n; p.desc = d.ctypes.data if n else None; p.levelsup = lv[i]; p.bow_n = -1
            for name, v in o.items():
                setattr(p, name, v.ctypes.data)
            keep.append((d, o, n))
        if nf == 0:
            return []
        rc = lib.ps_bow_transform(matcher._h, self._h, arr, nf)
        if not (partial_ok and rc == -3):
            check(rc)
        res = []
        for i, (d, o, n) in enumerate(keep):
            m = arr[i].bow_n
            res.append(dict(word=o["word"][:n].copy(), node=o["node"][:n].copy(), bow_id=o["bow_id"][:max(m, 0)].copy(),
                            bow_val=o["bow_val"][:max(m, 0)].copy(), failed=m < 0))
        return res


def feature_vector(node):
    """DBoW2::FeatureVector from node[]: {node id: [feature indices, ascending]} - addFeature's order"""
    fv = {}
    for i, v in enumerate(np.asarray(node)):
        if v >= 0:
            fv.setdefault(int(v), []).append(i)
    return fv


def synthetic_vocabulary(seed, k=10, L=3, p_prune=0.0, p_stop=0.0, tie_siblings=0.0, weighting=TF_IDF):
    """A seeded tree in record (breadth-first) order, as arrays for Vocabulary.from_arrays / save_binary.  Every inner node has
    k children with random descriptors; below the first level a node turns into a leaf early with probability p_prune (leaves
    at several depths), a leaf's weight is zero with probability p_stop (a stopped word), and with probability tie_siblings
    the second child of a node repeats the first child's descriptor (a tie the descent must break towards the first)."""
    rng = synth.Rng(seed)
    parent, desc, weight, leaf, depth = [], [], [], [], []
    inner = np.zeros(1, np.int64)          # node ids to expand at this level; the root is node 0
    next_id = 1
    for d in range(1, L + 1):
        m = len(inner) * k
        if m == 0:
            break
        par = np.repeat(inner, k)
        dsc = (rng.u64(m * 4).view(np.uint8)).reshape(m, 32).copy()
        tie = np.nonzero(rng.uniform(len(inner)) < tie_siblings)[0] if k > 1 else np.zeros(0, np.int64)
        dsc[tie * k + 1] = dsc[tie * k]
        is_leaf = np.ones(m, bool) if d == L else (rng.uniform(m) < p_prune)
        w = np.where(is_leaf, rng.uniform(m, 0.1, 5.0), 0.0)
        w = np.where(is_leaf & (rng.uniform(m) < p_stop), 0.0, w)
        ids = next_id + np.arange(m)
        next_id += m
        parent.append(par); desc.append(dsc); weight.append(w); leaf.append(is_leaf); depth.append(np.full(m, d))
        inner = ids[~is_leaf]
    return dict(k=k, L=L, weighting=weighting, parent=np.concatenate(parent).astype(np.int32), desc=np.concatenate(desc),
                weight=np.concatenate(weight).astype(np.float32), is_leaf=np.concatenate(leaf).astype(np.uint8),
                depth=np.concatenate(depth).astype(np.int32))
