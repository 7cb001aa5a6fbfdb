"""ctypes wrapper of tests/cpu_sim/viz_carry_sim.cpp (g++ build of viz_schedule in csrc/adder_viz_player_logic.hpp,
driven call after call with a small ring and carried state) -- test helper."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "adder-codec-rs_amd", "csrc")
_SRC = os.path.join(_HERE, "cpu_sim", "viz_carry_sim.cpp")
_LIB = os.path.join(_HERE, "cpu_sim", "libadder_viz_carry_sim.so")
_lib = None

REFUSED = -2  # a fill reaches frame w0 + ring: the player's depth refusal


def lib():
    global _lib
    if _lib is None:
        deps = [_SRC, os.path.join(_CSRC, "adder_viz_player_logic.hpp")]
        if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", _CSRC, _SRC,
                                   "-o", _LIB])
        L = C.CDLL(_LIB)
        vp, u32, i32, u64 = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64
        L.vcs_call.restype = C.c_int64
        L.vcs_call.argtypes = [vp, vp, vp, vp, u64, u32, u32, u32, i32, i32, vp, vp, C.c_int, u32, C.c_int, C.c_int, vp,
                               vp, u64, vp, vp]
        _lib = L
    return _lib


class CarrySim:
    """The schedule's carried state over the calls of one stream: frames_written, M, cnt [rows * ring], done [rows],
    the global event count and whether the limit was set since the last call."""

    def __init__(self, rows, row_units, ring, buffer_limit):
        self.rows, self.row_units, self.ring, self.limit = rows, row_units, ring, buffer_limit
        self.w, self.m, self.n_events, self.limit_set = 0, -1, 0, False
        self.cnt = np.zeros(rows * ring, np.uint32)
        self.done = np.zeros(rows, np.uint8)

    def set_buffer_limit(self, buffer_limit):
        self.limit, self.limit_set = buffer_limit, True

    def call(self, row, frm, to, last, finish=False):
        """-> (global P of the frames popped, flushed marks), or REFUSED with nothing changed"""
        arr = [np.ascontiguousarray(a, dtype=np.int32) for a in (row, frm, to, last)]
        n = len(arr[0])
        pops, fl = np.zeros(self.ring + 1, np.int32), np.zeros(self.ring + 1, np.uint8)
        w_end, m_end = C.c_int32(0), C.c_int32(0)
        k = lib().vcs_call(*[a.ctypes.data for a in arr], n, self.rows, self.row_units, self.ring, self.w, self.m,
                           self.cnt.ctypes.data, self.done.ctypes.data, 0 if self.limit is None else 1, self.limit or 0,
                           1 if self.limit_set else 0, 1 if finish else 0, pops.ctypes.data, fl.ctypes.data, len(pops),
                           C.byref(w_end), C.byref(m_end))
        if k == REFUSED:
            return REFUSED
        if k < 0:
            raise ValueError("vcs_call refused its arguments")
        out = [self.n_events + int(p) for p in pops[:k]]
        assert w_end.value == self.w + k
        self.w, self.m, self.n_events, self.limit_set = w_end.value, m_end.value, self.n_events + n, False
        return out, fl[:k].copy()
