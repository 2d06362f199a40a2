"""Host-side mirror of the frame handle (ps_frame, include/pointslot_hip.h): a stereo Frame's search-relevant state - mvKeysUn,
mvuRight, mDescriptors and mGrid (/root/reference/src/Frame.cc:709-722, 1636-1656) - kept on the device between the calls that
search into it.  ORBmatcher.SearchByProjection / FuseSearch take one as pr["train"]["frame"]."""
import ctypes

import numpy as np

from ._lib import lib, check
from .extractor import KEYPOINT_DTYPE

FRAME_NCELL = 64 * 48

lib.ps_frame_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
lib.ps_frame_destroy.argtypes = [ctypes.c_void_p]
lib.ps_frame_destroy.restype = None
lib.ps_frame_publish_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float]
lib.ps_frame_publish_orb.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float]
lib.ps_frame_count.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
lib.ps_frame_last_publish_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
lib.ps_frame_debug_read.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]

_READ = (("x", np.float32, 1), ("y", np.float32, 1), ("octave", np.int32, 1), ("angle", np.float32, 1), ("u_right", np.float32, 1),
         ("desc", np.uint8, 32))


def keypoints_from(x, y, octave, angle):
    """a cv::KeyPoint array (mvKeysUn) from the four members the matchers read"""
    k = np.zeros(len(x), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = x, y, octave, angle
    k["class_id"] = -1
    return k


def publish_many(frames, extractor, image, pair, n, grid):
    """ps_frame_publish_orb: several handles from one extractor's device-resident results in one launch."""
    arr = (ctypes.c_void_p * len(frames))(*[f._h.value for f in frames])
    im = np.ascontiguousarray(image, np.int32); pr = np.ascontiguousarray(pair, np.int32); nn = np.ascontiguousarray(n, np.int32)
    if not (len(im) == len(pr) == len(nn) == len(frames)):
        raise ValueError("one image / pair / n entry per frame handle")
    check(lib.ps_frame_publish_orb(arr, len(frames), extractor._h, im.ctypes.data, pr.ctypes.data, nn.ctypes.data, *[float(v) for v in grid]))


class DeviceFrame:
    """ps_frame: `capacity` keypoints at most (<= 32767).  A tracker keeps two (current frame, last frame) and alternates."""

    def __init__(self, capacity, device=0):
        self._h = ctypes.c_void_p()
        self.capacity = int(capacity)
        check(lib.ps_frame_create(device, self.capacity, ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib.ps_frame_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = ctypes.c_int(0)
        check(lib.ps_frame_count(self._h, ctypes.byref(n)))
        return n.value

    def publish(self, kps, u_right, desc, grid):
        """kps: mvKeysUn as a KEYPOINT_DTYPE array (or a dict with x, y, octave, angle); u_right: mvuRight or None (monocular);
        desc: mDescriptors [n, 32]; grid: (mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv).  Asynchronous."""
        if isinstance(kps, dict):
            kps = keypoints_from(kps["x"], kps["y"], kps["octave"], kps["angle"])
        k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        if len(d) != len(k) or (ur is not None and len(ur) != len(k)):
            raise ValueError("keypoints, u_right and descriptors differ in length")
        check(lib.ps_frame_publish_host(self._h, k.ctypes.data, None if ur is None else ur.ctypes.data, d.ctypes.data, len(k),
                                        *[float(v) for v in grid]))

    def publish_from(self, extractor, image, pair, n, grid):
        """From the extractor's last results, still on the device: image = the left image's index in its batch, pair = its index
        in the stereo outputs (-1: none), n = the keypoint count already fetched.  No host round trip."""
        publish_many([self], extractor, [image], [pair], [n], grid)

    def last_publish_ms(self):
        v = ctypes.c_float(0)
        check(lib.ps_frame_last_publish_ms(self._h, ctypes.byref(v)))
        return v.value

    def read(self):
        """blocking debug read-back: dict of x, y, octave, angle, u_right, desc, cell_off, cell_idx (all n entries: the lists,
        then zeros for keypoints outside the grid)"""
        out = {}
        n = ctypes.c_int(0)
        for what, (name, dt, width) in enumerate(_READ):
            a = np.zeros((self.capacity, width) if width > 1 else self.capacity, dt)
            check(lib.ps_frame_debug_read(self._h, what, a.ctypes.data, a.nbytes, ctypes.byref(n)))
            out[name] = a[:n.value].copy()
        off = np.zeros(FRAME_NCELL + 1, np.int32)
        check(lib.ps_frame_debug_read(self._h, 6, off.ctypes.data, off.nbytes, ctypes.byref(n)))
        idx = np.zeros(self.capacity, np.int32)
        check(lib.ps_frame_debug_read(self._h, 7, idx.ctypes.data, idx.nbytes, ctypes.byref(n)))
        out["cell_off"], out["cell_idx"], out["n"] = off, idx[:n.value].copy(), n.value
        return out
