"""ctypes binding of the C++ mirror's FeatureTracker (adder-codec-rs_amd/host, adder_host_features_*) -- test helper.

`MirrorFramer` offers what framer_features_cases.run drives.  The tracker is the reference's serial loop on the host and
holds no frames (those live on the device): the frames, and with them frames_written, come from a restatement that is
fed the same events with detection off."""
import ctypes as C
import os

import numpy as np

import framer_features_oracle as R

_PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adder-codec-rs_amd")
_lib = None


def lib():
    global _lib
    if _lib is None:
        import adder_amd
        adder_amd.load()  # libadder_host.so links libadder_hip.so
        L = C.CDLL(os.path.join(_PKG, "host", "libadder_host.so"))
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.adder_host_features_new.restype = vp
        L.adder_host_features_new.argtypes = [C.c_uint16, C.c_uint16, C.c_uint8, vp, C.c_float, C.c_float]
        L.adder_host_features_free.argtypes = [vp]
        L.adder_host_features_detect.argtypes = [vp, C.c_int]
        L.adder_host_features_ingest.restype = C.c_longlong
        L.adder_host_features_ingest.argtypes = [vp, vp, u64, C.POINTER(C.c_int), C.POINTER(u32), C.c_longlong, u64, vp]
        L.adder_host_features_pop.restype = C.c_int
        L.adder_host_features_pop.argtypes = [vp, C.POINTER(u64), vp, u32, C.POINTER(u32)]
        L.adder_host_features_plane.argtypes = [vp, vp]
        _lib = L
    return _lib


class MirrorFramer:
    def __init__(self, **params):
        self.L = lib()
        self.frames = R.Restatement(**params)  # frames and frames_written only: detection stays off in it
        p = dict(params)
        arr = np.array([p["tps"], p["ref_interval"], p["delta_t_max"], p.get("codec_version", 1), p.get("time_mode", 0),
                        p.get("view_mode", 0), p.get("source_type", 0), p.get("value_type", 0), p.get("source_camera", 0)],
                       np.uint32)
        self.w, self.h_, self.ch = p["width"], p["height"], p["channels"]
        self.h = self.L.adder_host_features_new(self.w, self.h_, self.ch, arr.ctypes.data, p.get("output_fps") or 0.0,
                                                p.get("practical_d_max", 0.0))
        assert self.h
        self.value_type_log2 = p.get("value_type", 0)
        self.detect = False
        self.last_valid, self.last_t = C.c_int(0), C.c_uint32(0)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.adder_host_features_free(self.h)
            self.h = None

    def detect_features(self, on):
        self.detect = bool(on)
        self.L.adder_host_features_detect(self.h, int(on))

    def reset_last_event(self):
        self.last_valid.value = 0

    def ingest(self, events, index_base=0):
        events = np.ascontiguousarray(events, R.EVENT_DTYPE)
        out = np.zeros(len(events), R.FEATURE_DTYPE)
        # the carried last event is the business of calls made with detection on (include/adder_framer.h)
        lv, lt = (self.last_valid, self.last_t) if self.detect else (C.c_int(0), C.c_uint32(0))
        n = self.L.adder_host_features_ingest(self.h, events.ctypes.data, len(events), C.byref(lv), C.byref(lt),
                                              self.frames.frames_written, index_base, out.ctypes.data)
        self.frames.ingest(events)
        return out[:n]

    def pop(self):
        return self.frames.pop()

    def write_frame_bytes(self):
        return self.frames.write_frame_bytes()

    def pop_features(self):
        end_ts, n = C.c_uint64(0), C.c_uint32(0)
        xy = np.zeros((1 << 16, 2), np.uint16)
        rc = self.L.adder_host_features_pop(self.h, C.byref(end_ts), xy.ctypes.data, len(xy), C.byref(n))
        if rc == 1:
            raise R.DequeBroken("panic")
        assert rc == 0
        return end_ts.value, xy[: n.value].copy()

    def running_intensities(self):
        out = np.zeros((self.h_, self.w, self.ch), np.uint8)
        self.L.adder_host_features_plane(self.h, out.ctypes.data)
        return out
