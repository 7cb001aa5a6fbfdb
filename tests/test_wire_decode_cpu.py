"""csrc/adder_wire.hpp -- the one decoder of AdderEvents and 9 / 11-byte wire records that the DVS converter, the stream
tools and both players run in their kernels -- built by g++ (tests/cpu_sim/wire_sim.cpp) and checked against the
independent numpy reader tests/adder_stream_np.py on hand-built records.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adder_stream_np as S

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "adder-codec-rs_amd", "csrc")
_SRC = os.path.join(_HERE, "cpu_sim", "wire_sim.cpp")
_LIB = os.path.join(_HERE, "cpu_sim", "libadder_wire_sim.so")
SRC_EVENTS, SRC_WIRE9, SRC_WIRE11 = 0, 1, 2

# an 11-byte record whose tag is not 1, as raw/stream.rs:177-201 reads it: d and t move up one byte, byte 10 is spare
WIRE11_NONE = np.dtype([("x", ">u2"), ("y", ">u2"), ("some", "u1"), ("d", "u1"), ("t", ">u4"), ("spare", "u1")])
assert WIRE11_NONE.itemsize == S.WIRE11.itemsize == 11 and S.WIRE9.itemsize == 9


@pytest.fixture(scope="module")
def sim():
    deps = [_SRC, os.path.join(_CSRC, "adder_wire.hpp"),
            os.path.join(os.path.dirname(_HERE), "include", "adder_hip.h")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-I", _CSRC, _SRC,
                               "-o", _LIB])
    L = C.CDLL(_LIB)
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    L.ws_load.restype, L.ws_load.argtypes = C.c_int, [C.c_int, vp, u64, vp]
    L.ws_record_bytes.restype, L.ws_record_bytes.argtypes = u64, [C.c_int]
    L.ws_source.restype, L.ws_source.argtypes = C.c_int, [u32]
    L.ws_t_offset.restype, L.ws_t_offset.argtypes = u32, [u32]
    L.ws_round_up.restype, L.ws_round_up.argtypes = u64, [u64, u64]
    L.ws_limit.restype, L.ws_limit.argtypes = u64, [u64, u64]
    return L


def load(L, source, body, n, offset):
    """The decoder over `body` placed `offset` bytes into a larger array -> uint32 [n, 6]: x, y, c, d, t, end"""
    big = np.full(len(body) + 16, 0xA5, np.uint8)
    base = (-big.ctypes.data) % 8  # an 8-byte aligned start, so that `offset` is the misalignment
    big[base + offset: base + offset + len(body)] = np.frombuffer(body, np.uint8)
    out = np.full((n, 6), 0xFFFFFFFF, np.uint32)
    assert L.ws_load(source, big.ctypes.data + base + offset, n, out.ctypes.data) == 1
    return out


# x, y, d, t of sixteen 9-byte records
WIRE9_RECORDS = [
    (1, 2, 7, 0x01020304),            # t: four distinct bytes
    (0x0102, 0x0304, 0, 0),           # x, y: two distinct bytes each
    (0xFFFF, 0xFFFF, 0, 0),           # the EOF pair: end
    (0xFFFF, 5, 3, 9),                # x alone: not end
    (6, 0xFFFF, 3, 9),                # y alone: not end
    (0xFFFF, 0xFFFF, 255, 0xFFFFFFFF),  # end whatever follows the pair
    (0, 0, 128, 0x80000000),
    (0xFFFE, 0xFFFF, 129, 0xDEADBEEF),
    (0xFFFF, 0xFFFE, 254, 0x0000FF00),
    (65, 66, 255, 0xFF000000),
    (67, 68, 127, 0x00FF0000),
    (69, 70, 1, 0x000000FF),
    (0x8000, 0x0080, 2, 0x7FFFFFFF),
    (0x00FF, 0xFF00, 4, 1),
    (9, 9, 9, 0x09090909),
    (0x1234, 0x5678, 0x9A, 0xBCDEF012),
]

# x, y, tag, then (c, d, t) for tag 1 or (d, t, spare) otherwise: sixteen 11-byte records
WIRE11_RECORDS = [
    (1, 2, 1, (2, 7, 0x01020304)),               # a tag-1 record, t of four distinct bytes
    (3, 4, 0, (9, 0x0A0B0C0D, 0x5A)),            # tag 0 with a non-zero byte 10: d from 5, t from 6..9
    (5, 6, 2, (11, 0x11121314, 0x15)),           # tag 2: end
    (7, 8, 255, (13, 0x21222324, 0x25)),         # tag 255: end
    None,                                        # adder_stream_np.EOF: x = y = 0xffff, tag 1: end
    (0xFFFF, 5, 1, (1, 3, 9)),                   # x alone: not end
    (6, 0xFFFF, 1, (1, 3, 9)),                   # y alone: not end
    (0xFFFF, 0xFFFF, 0, (3, 0x31323334, 0)),     # the EOF pair behind tag 0: end
    (0x0102, 0x0304, 1, (0, 128, 0)),
    (10, 11, 1, (255, 255, 0xFFFFFFFF)),         # Some(255) on the wire is channel 255, not None
    (12, 13, 0, (128, 0xDEADBEEF, 0xFF)),
    (14, 15, 1, (1, 0, 0x80000000)),
    (16, 17, 0, (255, 0, 1)),                    # tag 0 whose byte 10 is 1: not a tag
    (0xFFFE, 0xFFFF, 1, (2, 254, 0x0000FF00)),
    (0xFFFF, 0xFFFE, 0, (129, 0x00FF00FF, 7)),
    (0x1234, 0x5678, 1, (0x9A, 0xBC, 0xDEF01234)),
]


def wire9_body():
    w = np.zeros(len(WIRE9_RECORDS), S.WIRE9)
    for i, (x, y, d, t) in enumerate(WIRE9_RECORDS):
        w[i] = (x, y, d, t)
    return w.tobytes()


def wire11_body():
    out = b""
    for rec in WIRE11_RECORDS:
        if rec is None:
            out += S.EOF
        elif rec[2] == 1:
            out += np.array([(rec[0], rec[1], 1) + rec[3]], S.WIRE11).tobytes()
        else:
            out += np.array([rec[:3] + rec[3]], WIRE11_NONE).tobytes()
    return out


def events_body():
    ev = np.zeros(16, S.EVENT_DTYPE)
    ev["x"] = [1, 0x0102, 0xFFFF, 0xFFFF, 6, 0, 0xFFFE, 65, 67, 69, 0x8000, 0x00FF, 9, 0x1234, 2, 3]
    ev["y"] = [2, 0x0304, 0xFFFF, 5, 0xFFFF, 0, 0xFFFF, 66, 68, 70, 0x0080, 0xFF00, 9, 0x5678, 2, 3]
    ev["c"] = [0xFF, 2, 0xFF, 1, 0, 2, 0xFE, 0xFF, 1, 2, 0, 1, 2, 0xFF, 3, 0x80]  # 0xff: None
    ev["d"] = [7, 0, 255, 3, 3, 128, 129, 254, 127, 1, 2, 4, 9, 0x9A, 0, 255]
    ev["pad"] = [0, 0xFFFF, 0x1234, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]  # carried by nothing
    ev["t"] = [0x01020304, 0, 0xFFFFFFFF, 9, 9, 0x80000000, 0xDEADBEEF, 0x0000FF00, 0xFF000000, 0x00FF0000,
               0x000000FF, 0x7FFFFFFF, 1, 0xBCDEF012, 0x09090909, 0x10203040]
    return ev


@pytest.mark.parametrize("offset", (0, 1, 2, 3))
def test_wire9_records_decode_as_the_numpy_reader_reads_them(sim, offset):
    body = wire9_body()
    got = load(sim, SRC_WIRE9, body, 16, offset)
    w = np.frombuffer(body, S.WIRE9)
    ev, tag, spare, end = S.decode_records(body, 1)
    for k, want in (("x", 0), ("y", 1), ("d", 3), ("t", 4)):
        assert np.array_equal(got[:, want], w[k]) and np.array_equal(got[:, want], ev[k]), k
    assert np.all(got[:, 2] == 0)  # no channel on the wire: channel 0
    ends = (w["x"] == 0xFFFF) & (w["y"] == 0xFFFF)
    assert np.array_equal(got[:, 5], ends) and list(np.flatnonzero(ends)) == [2, 5] and end == 2
    assert got[0, 4] == 0x01020304 and got[1, 0] == 0x0102 and got[1, 1] == 0x0304


@pytest.mark.parametrize("offset", (0, 1, 2, 3))
def test_wire11_records_decode_by_their_tag(sim, offset):
    body = wire11_body()
    assert len(body) == 16 * 11 and body[4 * 11: 5 * 11] == S.EOF
    got = load(sim, SRC_WIRE11, body, 16, offset)
    some_view, none_view = np.frombuffer(body, S.WIRE11), np.frombuffer(body, WIRE11_NONE)
    tag = some_view["some"]
    some = tag == 1
    assert np.array_equal(got[:, 0], some_view["x"]) and np.array_equal(got[:, 1], some_view["y"])
    assert np.array_equal(got[:, 2], np.where(some, some_view["c"], 0))
    assert np.array_equal(got[:, 3], np.where(some, some_view["d"], none_view["d"]))
    assert np.array_equal(got[:, 4], np.where(some, some_view["t"], none_view["t"]))
    ends = (tag > 1) | ((some_view["x"] == 0xFFFF) & (some_view["y"] == 0xFFFF))
    assert np.array_equal(got[:, 5], ends) and list(np.flatnonzero(ends)) == [2, 3, 4, 7]
    # the reader's own tag-aware decode says the same (its c = 0xff stands for None)
    ev, dtag, spare, end = S.decode_records(body, 3)
    assert end == 2 and np.array_equal(dtag, tag)
    for k, col in (("x", 0), ("y", 1), ("d", 3), ("t", 4)):
        assert np.array_equal(got[:, col], ev[k]), k
    assert np.array_equal(got[:, 2], np.where(some, ev["c"], 0))
    # the named cases, by value
    assert tuple(got[0]) == (1, 2, 2, 7, 0x01020304, 0)
    assert tuple(got[1]) == (3, 4, 0, 9, 0x0A0B0C0D, 0) and spare[1] == 0x5A
    assert got[2, 5] == 1 and got[3, 5] == 1 and got[4, 5] == 1
    assert tuple(got[5, [0, 1, 5]]) == (0xFFFF, 5, 0) and tuple(got[6, [0, 1, 5]]) == (6, 0xFFFF, 0)
    assert tuple(got[9]) == (10, 11, 255, 255, 0xFFFFFFFF, 0)
    assert tuple(got[12]) == (16, 17, 0, 255, 0, 0) and spare[12] == 1
    for t in range(256):
        assert sim.ws_t_offset(t) == (7 if t == 1 else 6)


@pytest.mark.parametrize("offset", (0, 1, 2, 3))
def test_adder_events_decode_with_none_as_channel_0(sim, offset):
    # (the library's entry points take AdderEvents at their type's alignment; the decoder itself is seen here not to
    # ask for more than the host gives)
    ev = events_body()
    got = load(sim, SRC_EVENTS, ev.tobytes(), 16, offset)
    for k, col in (("x", 0), ("y", 1), ("d", 3), ("t", 4)):
        assert np.array_equal(got[:, col], ev[k]), k
    assert np.array_equal(got[:, 2], np.where(ev["c"] == 0xFF, 0, ev["c"]))
    assert got[0, 2] == 0 and got[1, 2] == 2 and got[6, 2] == 0xFE
    assert np.all(got[:, 5] == 0)  # an AdderEvent never ends the stream, x = y = 0xffff included
    assert got[2, 0] == 0xFFFF and got[2, 1] == 0xFFFF


def test_source_and_record_bytes(sim):
    assert [sim.ws_record_bytes(s) for s in (SRC_EVENTS, SRC_WIRE9, SRC_WIRE11)] == [S.EVENT_DTYPE.itemsize, 9, 11]
    assert sim.ws_source(1) == SRC_WIRE9 and sim.ws_source(3) == SRC_WIRE11 and sim.ws_source(2) == SRC_WIRE11
    assert sim.ws_load(3, None, 0, None) == 0


def test_round_up_and_limit(sim):
    ref = 255
    for t in (0, ref - 1, ref, ref + 1, 2 ** 32 - 1, 2 * ref, 2 ** 32 - 2, 2 ** 40 + 1):
        assert sim.ws_round_up(t, ref) == (t if t % ref == 0 else (t // ref + 1) * ref), t
    assert sim.ws_round_up(0, ref) == 0 and sim.ws_round_up(254, ref) == 255 and sim.ws_round_up(256, ref) == 510
    assert sim.ws_round_up(2 ** 32 - 1, ref) == 2 ** 32 - 1  # 255 * 16843009
    assert sim.ws_round_up(2 ** 32 - 2, ref) == 2 ** 32 - 1 and sim.ws_round_up(2 ** 32 - 1, 256) == 2 ** 32
    for t in (0, 1, 7, 2 ** 32 - 1):
        assert sim.ws_round_up(t, 1) == t
    none = 2 ** 64 - 1
    assert sim.ws_limit(3, 9) == 3 and sim.ws_limit(9, 3) == 3 and sim.ws_limit(5, 5) == 5
    assert sim.ws_limit(none, 16) == 16 and sim.ws_limit(0, 0) == 0
