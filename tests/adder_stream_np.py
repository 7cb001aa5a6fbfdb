"""Independent numpy reader/writer of the raw `.adder` container (test helper).

Follows adder-codec-core/src/codec/header.rs:14-25, encoder.rs:170-229 (header +
V1/V2/V3 extensions), raw/stream.rs:101-120 (9/11-byte big-endian events) and
raw/stream.rs:79-92 (11-byte EOF).  Written separately from oracle/adder_oracle.c
so the two can be diffed against each other and against the golden files.
"""
import struct

import numpy as np

EVENT_DTYPE = np.dtype(
    [("x", "<u2"), ("y", "<u2"), ("c", "u1"), ("d", "u1"), ("pad", "<u2"), ("t", "<u4")]
)
WIRE9 = np.dtype([("x", ">u2"), ("y", ">u2"), ("d", "u1"), ("t", ">u4")])
WIRE11 = np.dtype([("x", ">u2"), ("y", ">u2"), ("some", "u1"), ("c", "u1"), ("d", "u1"), ("t", ">u4")])
EOF = bytes([0xFF, 0xFF, 0xFF, 0xFF, 0x01, 0, 0, 0, 0, 0, 0])


def parse_header(buf):
    magic, version, endian, w, h, tps, ref, dtm, esize, ch = struct.unpack(">5sBBHHIIIBB", buf[:25])
    assert magic == b"adder" and endian == ord("b")
    meta = dict(version=version, width=w, height=h, tps=tps, ref_interval=ref, delta_t_max=dtm,
                event_size=esize, channels=ch, source_camera=0, time_mode=0, adu_interval=0)
    off = 25
    if version >= 1:
        (meta["source_camera"],) = struct.unpack(">I", buf[off:off + 4]); off += 4
    if version >= 2:
        (meta["time_mode"],) = struct.unpack(">I", buf[off:off + 4]); off += 4
    if version >= 3:
        (meta["adu_interval"],) = struct.unpack(">I", buf[off:off + 4]); off += 4
    meta["header_size"] = off
    return meta


def build_header(meta):
    b = struct.pack(">5sBBHHIIIBB", b"adder", meta["version"], ord("b"), meta["width"], meta["height"],
                    meta["tps"], meta["ref_interval"], meta["delta_t_max"],
                    9 if meta["channels"] == 1 else 11, meta["channels"])
    if meta["version"] >= 1:
        b += struct.pack(">I", meta["source_camera"])
    if meta["version"] >= 2:
        b += struct.pack(">I", meta["time_mode"])
    if meta["version"] >= 3:
        b += struct.pack(">I", meta["adu_interval"])
    return b


def read_adder(buf):
    """-> (meta, events[EVENT_DTYPE], closed: bool).  Stops at the EOF event."""
    meta = parse_header(buf)
    body = buf[meta["header_size"]:]
    es = meta["event_size"]
    closed = False
    if meta["channels"] == 1:
        # EOF is 11 bytes even here (raw/stream.rs:79-92); it starts with ff ff ff ff
        n = len(body) // es
        arr = np.frombuffer(body[: n * es], dtype=WIRE9)
        eof = np.nonzero((arr["x"] == 0xFFFF) & (arr["y"] == 0xFFFF))[0]
        if len(eof):
            n = int(eof[0])
            closed = body[n * es: n * es + 11] == EOF
        arr = arr[:n]
        ev = np.zeros(n, EVENT_DTYPE)
        ev["x"], ev["y"], ev["c"], ev["d"], ev["t"] = arr["x"], arr["y"], 0xFF, arr["d"], arr["t"]
    else:
        n = len(body) // es
        arr = np.frombuffer(body[: n * es], dtype=WIRE11)
        eof = np.nonzero((arr["x"] == 0xFFFF) & (arr["y"] == 0xFFFF))[0]
        if len(eof):
            n = int(eof[0])
            closed = True
        arr = arr[:n]
        assert np.all(arr["some"] == 1)
        ev = np.zeros(n, EVENT_DTYPE)
        ev["x"], ev["y"], ev["c"], ev["d"], ev["t"] = arr["x"], arr["y"], arr["c"], arr["d"], arr["t"]
    return meta, ev, closed


def write_adder(meta, events, close=True):
    out = build_header(meta)
    if meta["channels"] == 1:
        w = np.zeros(len(events), WIRE9)
        w["x"], w["y"], w["d"], w["t"] = events["x"], events["y"], events["d"], events["t"]
    else:
        w = np.zeros(len(events), WIRE11)
        w["x"], w["y"], w["some"], w["c"], w["d"], w["t"] = (
            events["x"], events["y"], 1, events["c"], events["d"], events["t"])
    out += w.tobytes()
    if close:
        out += EOF
    return out


# ---- tag-aware records (tests/stream_edge_cases.py) ---------------------------------------------------------------
# An 11-byte record is x, y, Option<u8> c, d, t as bincode lays them out, read back with a fixed 11-byte read
# (raw/stream.rs:177-201): tag 1 = Some(c): c at byte 5, d at 6, t at 7..10; tag 0 = None: d at byte 5, t at 6..9 and
# byte 10 belongs to nothing (`spare`, carried); a tag above 1 does not decode and ends the stream like the EOF
# record (x = y = 0xFFFF).  9-byte records have no tag; their c is None.

def decode_records(body, channels):
    """-> (events[EVENT_DTYPE] of EVERY whole record, tag u8[n], spare u8[n], end): c = 0xFF for tag 0 and for 9-byte
    records; `end` is the index of the first record that ends the stream, or n.  Records from `end` on are decoded by
    their tag's layout all the same (tag > 1: as None) so that a test can say what lay behind the end."""
    rb = 9 if channels == 1 else 11
    n = len(body) // rb
    b = np.frombuffer(bytes(body[: n * rb]), np.uint8).reshape(n, rb).astype(np.uint32)
    ev = np.zeros(n, EVENT_DTYPE)
    ev["x"], ev["y"] = (b[:, 0] << 8) | b[:, 1], (b[:, 2] << 8) | b[:, 3]
    tag, spare = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    if channels == 1:
        ev["c"], ev["d"], tb = 0xFF, b[:, 4], b[:, 5:9]
        ends = (ev["x"] == 0xFFFF) & (ev["y"] == 0xFFFF)
    else:
        tag = b[:, 4].astype(np.uint8)
        some = tag == 1
        ev["c"] = np.where(some, b[:, 5], 0xFF)
        ev["d"] = np.where(some, b[:, 6], b[:, 5])
        tb = np.where(some[:, None], b[:, 7:11], b[:, 6:10])
        spare = np.where(some, 0, b[:, 10]).astype(np.uint8)
        ends = (tag > 1) | ((ev["x"] == 0xFFFF) & (ev["y"] == 0xFFFF))
    ev["t"] = (tb[:, 0] << 24) | (tb[:, 1] << 16) | (tb[:, 2] << 8) | tb[:, 3]
    hit = np.flatnonzero(ends)
    return ev, tag, spare, int(hit[0]) if len(hit) else n


def encode_records(events, channels, tag=None, spare=None):
    """The inverse of decode_records on records of tag 0 and 1.  tag None: Some(c), except None where c == 0xFF."""
    n = len(events)
    be = lambda v, k: [((v.astype(np.uint32) >> s) & 0xFF).astype(np.uint8) for s in range(8 * k - 8, -8, -8)]
    cols = be(events["x"], 2) + be(events["y"], 2)
    d, t = events["d"].astype(np.uint8), be(events["t"], 4)
    if channels == 1:
        cols += [d] + t
    else:
        tag = np.where(events["c"] == 0xFF, 0, 1).astype(np.uint8) if tag is None else np.asarray(tag, np.uint8)
        spare = np.zeros(n, np.uint8) if spare is None else np.asarray(spare, np.uint8)
        assert np.all(tag <= 1) and np.all(events["c"][tag == 0] == 0xFF)
        some = tag == 1
        cols += [tag, np.where(some, events["c"], d), np.where(some, d, t[0]), np.where(some, t[0], t[1]),
                 np.where(some, t[1], t[2]), np.where(some, t[2], t[3]), np.where(some, t[3], spare)]
    return np.stack(cols, 1).tobytes() if n else b""
