"""ctypes wrapper of tests/cpu_sim/framer_features_sim.cpp (g++ build of csrc/adder_framer_features.hpp) -- test helper.

`SimFramer` offers what framer_features_cases.run drives.  The per-event logic and the sort / search / commit shape
are the device's; the FeatureInterval deque, which the library keeps on the host in plain C++, is borrowed from the
restatement here (it is not device logic)."""
import ctypes as C
import os
import subprocess

import numpy as np

import framer_features_oracle as R

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "adder-codec-rs_amd", "csrc")
_SRC = os.path.join(_HERE, "cpu_sim", "framer_features_sim.cpp")
_LIB = os.path.join(_HERE, "cpu_sim", "libadder_framer_features_sim.so")
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    deps = [_SRC] + [os.path.join(_CSRC, n) for n in ("adder_framer_features.hpp", "adder_framer.hpp", "adder_pixel.hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra",
                               "-I", _CSRC, _SRC, "-o", _LIB])
    L = C.CDLL(_LIB)
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    L.ffs_new.restype = vp
    L.ffs_new.argtypes = [u32, u32, u32, u32, u32, u32, u32, u32, u32, f32, u32, u32]
    L.ffs_free.argtypes = [vp]
    L.ffs_detect.argtypes = [vp, C.c_int]
    L.ffs_reset_last_event.argtypes = [vp]
    L.ffs_frames_written.restype = C.c_int64
    L.ffs_frames_written.argtypes = [vp]
    L.ffs_plane.argtypes = [vp, vp]
    L.ffs_ingest.restype = C.c_int64
    L.ffs_ingest.argtypes = [vp, vp, u32, u64, vp]
    L.ffs_pop_frame.restype = C.c_int
    L.ffs_pop_frame.argtypes = [vp, vp, C.c_int]
    L.ffs_fast9_ring16_plane.argtypes = [vp, u32, u32, u32, vp]
    _lib = L
    return L


def fast9_ring16_plane(img):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    out = np.zeros((h, w), np.uint8)
    lib().ffs_fast9_ring16_plane(img.ctypes.data, w, h, ch, out.ctypes.data)
    return out


class SimFramer:
    def __init__(self, **params):
        self.L = lib()
        self.r = R.Restatement(**params)  # parameters (tpf, abs_t, round_up) and the deque only
        r = self.r
        self.h = self.L.ffs_new(r.w, r.h, r.ch, r.tpf, r.ref_interval, int(r.abs_t), int(r.round_up), r.view, r.source,
                                r.pdm, r.delta_t_max, r.vt)
        self.value_type_log2 = r.vt
        self.detect = False

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ffs_free(self.h)
            self.h = None

    def detect_features(self, on):
        self.detect = bool(on)
        self.L.ffs_detect(self.h, int(on))

    def reset_last_event(self):
        self.L.ffs_reset_last_event(self.h)

    def ingest(self, events, index_base=0):
        events = np.ascontiguousarray(events, R.EVENT_DTYPE)
        out = np.zeros(len(events), R.FEATURE_DTYPE)
        n = self.L.ffs_ingest(self.h, events.ctypes.data, len(events), index_base, out.ctypes.data)
        assert n >= 0, "an event outside the plane"
        self.r.frames_written = self.L.ffs_frames_written(self.h)
        for f in out[:n]:
            self.r._file(int(f["t"]), int(f["x"]), int(f["y"]))
        return out[:n]

    def _frame(self, complete_only):
        r = self.r
        buf = np.zeros(r.w * r.h * r.ch, np.uint32)
        if not self.L.ffs_pop_frame(self.h, buf.ctypes.data, complete_only):
            return None
        return buf.astype((">u1", ">u2", ">u4")[r.vt]).tobytes()

    def pop(self):
        out = []
        while True:
            f = self._frame(1)
            if f is None:
                return b"".join(out)
            out.append(f)

    def write_frame_bytes(self):
        return self._frame(0)

    def pop_features(self):
        return self.r.pop_features()

    def running_intensities(self):
        r = self.r
        out = np.zeros((r.h, r.w, r.ch), np.uint8)
        self.L.ffs_plane(self.h, out.ctypes.data)
        return out
