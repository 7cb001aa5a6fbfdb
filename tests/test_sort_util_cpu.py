"""The pure rules the event tools' *_api.cpp share (adder-codec-rs_amd/csrc/adder_sort_util.hpp): the radix bits of a
unit key, the scratch a call's records take, the Crf table.  The header is the one libadder_hip.so compiles; g++ builds
it here with a small C shim (tests/cpu_sim/sort_util.cpp), so it is also held to compiling without HIP."""
import ctypes as C
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "adder-codec-rs_amd", "csrc")
_SRC = os.path.join(_HERE, "cpu_sim", "sort_util.cpp")
_LIB = os.path.join(_HERE, "cpu_sim", "libadder_sort_util.so")
_DEPS = [_SRC, os.path.join(_CSRC, "adder_sort_util.hpp")]

INT32_MAX = (1 << 31) - 1

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in _DEPS):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                                   "-I", _CSRC, _SRC, "-o", _LIB])
        L = C.CDLL(_LIB)
        L.sort_util_key_bits.restype = C.c_uint32
        L.sort_util_key_bits.argtypes = [C.c_uint64]
        L.sort_util_scratch_capacity.restype = C.c_uint64
        L.sort_util_scratch_capacity.argtypes = [C.c_uint64]
        L.sort_util_crf_row.argtypes = [C.c_int, C.POINTER(C.c_uint8)]
        _lib = L
    return _lib


UNITS = [1, 2, 3, 4] + [v for k in (8, 16, 20, 31) for v in ((1 << k) - 1, 1 << k)] + [(1 << 32) - 2]


@pytest.mark.parametrize("units", UNITS)
def test_key_bits_for(units):
    """The smallest b >= 1 with 2^b >= units + 1: keys 0..units fit in b bits."""
    b = lib().sort_util_key_bits(units)
    assert b == max(1, units.bit_length())
    assert (1 << b) >= units + 1 and (b == 1 or (1 << (b - 1)) < units + 1)


# the largest n with n + n // 8 <= 2^31 - 1
EDGE = max(n for n in range(INT32_MAX * 8 // 9 - 2, INT32_MAX * 8 // 9 + 3) if n + n // 8 <= INT32_MAX)


@pytest.mark.parametrize("n", [0, 7, 8, 9, EDGE, EDGE + 1, INT32_MAX, 1 << 40])
def test_scratch_capacity(n):
    assert lib().sort_util_scratch_capacity(n) == min(n + n // 8, INT32_MAX)


def test_scratch_capacity_edge_is_the_edge():
    assert EDGE + EDGE // 8 <= INT32_MAX < (EDGE + 1) + (EDGE + 1) // 8


def test_crf_table_is_the_bindings_and_the_oracles():
    import prophesee_oracle
    from adder_amd.video import CRF
    L = lib()
    assert L.sort_util_crf_rows() == len(CRF) == len(prophesee_oracle.CRF) == 10
    for q in range(10):
        row = (C.c_uint8 * 3)()
        L.sort_util_crf_row(q, row)
        assert tuple(row) == tuple(CRF[q]) == tuple(prophesee_oracle.CRF[q])
