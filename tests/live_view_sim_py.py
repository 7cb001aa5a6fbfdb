"""ctypes wrapper of tests/cpu_sim/live_view_sim.cpp (g++ build of the live view's functions in csrc/adder_pixel.hpp) --
test helper."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "adder-codec-rs_amd", "csrc")
_SRC = os.path.join(_HERE, "cpu_sim", "live_view_sim.cpp")
_LIB = os.path.join(_HERE, "cpu_sim", "libadder_live_view_sim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [_SRC, os.path.join(_CSRC, "adder_pixel.hpp")]
        if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra",
                                   "-I", _CSRC, _SRC, "-o", _LIB])
        L = C.CDLL(_LIB)
        vp, u32 = C.c_void_p, C.c_uint32
        L.lvs_values.argtypes = [u32, u32, u32, C.c_float, vp, vp, vp, vp, C.c_size_t, vp]
        L.lvs_display.argtypes = [vp, vp, u32, u32, u32, vp]
        _lib = L
    return _lib


def values(view, ref_time, delta_t_max, practical_d_max, d, t, clock, prev):
    d, t, clock, prev = (np.ascontiguousarray(np.broadcast_to(a, np.broadcast(d, t, clock, prev).shape), np.uint32).reshape(-1)
                         for a in (d, t, clock, prev))
    out = np.zeros(len(d), np.uint8)
    lib().lvs_values(view, ref_time, delta_t_max, practical_d_max, d.ctypes.data, t.ctypes.data, clock.ctypes.data,
                     prev.ctypes.data, len(d), out.ctypes.data)
    return out


def display(plane, member):
    plane = np.ascontiguousarray(plane, np.uint8)
    member = np.ascontiguousarray(member, np.uint8)
    h, w, ch = plane.shape
    out = np.zeros_like(plane)
    lib().lvs_display(plane.ctypes.data, member.ctypes.data, w, h, ch, out.ctypes.data)
    return out
