"""pointslot_amd — MI355X-native hot path (ORB front-end, Hamming matching, pose optimisation, object
bundle adjustment, bag of words, the keyframe database and the loop-closure Sim3 solver) behind the C-ABI of include/pointslot_hip.h.  No CPU fallback:
importing the operator modules requires libpointslot_hip.so."""
__version__ = "0.1.0"


def __getattr__(name):
    # the operator modules load the shared library on import, so the package itself stays importable without it
    if name == "KeyFrameDatabase":
        from .kfdb import KeyFrameDatabase
        return KeyFrameDatabase
    if name == "Sim3Solver":
        from .sim3solver import Sim3Solver
        return Sim3Solver
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
