"""Prophesee .dat -> ADDER (include/adder_prophesee.h) without a GPU: the library's header parser, record decoder,
group scan and host exp against the restatement (tests/prophesee_oracle.py), libm and hand-derived answers."""
import math
import random

import numpy as np
import pytest

import prophesee_oracle as R
from adder_amd import prophesee as P
from adder_amd._native import AdderHipError, E_BAD_PARAMS, E_OUT_CAPACITY

LN_MID = math.log1p(128.0 / 255.0)

HEADERS = [
    # (bytes, (width, height, header_bytes, ev_type, ev_size) or an error code)
    (b"", (100, 70, 0, 0, 0)),                                                   # no header at all: the defaults
    (b"\x01\x02", (100, 70, 0, 0, 0)),                                           # no '%' line: no type bytes
    (b"% Height 720\n% Width 1280\n\x00\x08", (1280, 720, 28, 0, 8)),
    (b"% Height 720\r\n% Width 1280\r\n\x0c\x08", (100, 70, 30, 12, 8)),         # "720\r" does not parse: defaults
    (b"%  Height 720\n% Width 64\n\x00\x08", (64, 70, 27, 0, 8)),                # double space: words[1] == ""
    (b"% Height\t33\n% Width\t+44\n\x00\x08", (44, 33, 26, 0, 8)),               # tab, a leading '+'
    (b"% Height 30\n% Height x\n\x00\x08", (100, 70, 25, 0, 8)),                 # a later bad value gives None
    (b"% Height 720\n", E_BAD_PARAMS),                                           # missing type bytes
    (b"% Height 720\n\x00", E_BAD_PARAMS),                                       # one type byte
    (b"% Height 720\n\x01\x08", E_BAD_PARAMS),                                   # bad ev_type
    (b"% Height 720\n\x00\x10", E_BAD_PARAMS),                                   # bad ev_size
    (b"% Width 0\n\x00\x08", E_BAD_PARAMS),                                      # width 0
    (b"% Width 65536\n\x00\x08", E_BAD_PARAMS),                                  # 0 after the u16 cast
    (b"% Width 65537\n\x00\x08", (1, 70, 16, 0, 8)),                             # 1 after the u16 cast
    (b"% Width 4294967296\n\x00\x08", (100, 70, 21, 0, 8)),                      # u32 overflow: None
    (b"% Height  9\n\x00\x08", E_BAD_PARAMS),                                    # empty words[2]: unwrap panics
    (b"% Width\n\x00\x08", (100, 70, 10, 0, 8)),                                 # words[1] == "Width\n"
    (b"% Width 12", E_BAD_PARAMS),                                               # the file ends in the header
    (b"%\n\n\x00\x08", E_BAD_PARAMS),                                           # "\n" ends the header: type bytes 0a 00
]


@pytest.mark.parametrize("data,want", HEADERS)
def test_header_table(data, want):
    if isinstance(want, int):
        with pytest.raises(AdderHipError) as ei:
            P.parse_header(data)
        assert ei.value.code == want
        with pytest.raises((R.BadHeader, ValueError)):
            bod, _, _, (h, w) = R.parse_header(data)
            R.plane_of(h, w)
        return
    got = P.parse_header(data)
    assert (got["width"], got["height"], got["header_bytes"], got["ev_type"], got["ev_size"]) == want
    bod, et, es, (h, w) = R.parse_header(data)
    assert (R.plane_of(h, w), bod, et, es) == ((want[0], want[1]), want[2], want[3], want[4])


def test_header_needs_more_of_the_file():
    data = b"% Height 720\n% Width 1280\n\x00\x08"
    with pytest.raises(AdderHipError) as ei:
        P.parse_header(data[:20], file_size=len(data))
    assert ei.value.code == E_OUT_CAPACITY
    assert P.parse_header(data[:28], file_size=1000)["header_bytes"] == 28


def test_record_decode_and_the_10_bit_x():
    rng = np.random.default_rng(3)
    t = rng.integers(0, 1 << 32, 5000)
    data = rng.integers(-(1 << 31), 1 << 31, 5000)
    raw = np.zeros(5000, P.RECORD_DTYPE)
    raw["t"], raw["data"] = t.astype(np.uint32), data.astype(np.int32)
    got = P.decode(raw)
    for i in range(5000):
        assert (got["t"][i], got["x"][i], got["y"][i], got["p"][i]) == R.decode_event(raw[i:i + 1].tobytes())
    # a 1280-wide sensor: x >= 1024 lands on x - 1024
    r = P.records([7, 8], [1100, 1279], [719, 3], [1, 0])
    got = P.decode(r)
    assert list(got["x"]) == [76, 255] and list(got["y"]) == [719, 3] and list(got["p"]) == [1, 0]


def _libm_exp(x):
    try:
        return math.exp(x)
    except OverflowError:  # libm returns inf (Python raises instead)
        return math.inf


def test_exp_equals_libm():
    rng = np.random.default_rng(11)
    xs = np.concatenate([
        rng.uniform(-500, 500, 4_000_000), rng.uniform(-1, 2, 4_000_000), rng.uniform(-750, 720, 1_000_000),
        rng.uniform(-1e-15, 1e-15, 100_000),
        # ln(128/255 + 1) +- k * 0.02: the chain's walk from the start intensity
        np.array([math.log1p(128.0 / 255.0) + s * k * 0.02 for k in range(1, 5000) for s in (1, -1)]),
        np.array([0.0, -0.0, 2.0 ** -54, -(2.0 ** -54), 2.0 ** -55, 511.999, 512.0, -512.0, 709.78, 709.79, -745.1,
                  -745.2, 1e308, -1e308, math.inf, -math.inf]),
    ])
    xs = np.concatenate([xs, rng.uniform(-0.7, 0.7, 10_000_000 - len(xs))])
    got = P.exp(xs)
    want = np.fromiter((_libm_exp(x) for x in xs), np.float64, len(xs))
    assert len(xs) >= 10_000_000
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert math.isnan(P.exp(math.nan))


def _scan(ts, start=2, rt=2):
    return P.scan_groups(P.records(ts, [0] * len(ts), [0] * len(ts), [0] * len(ts)), start, rt)


def test_group_scan_hand_cases():
    V = R.VIEW_INTERVAL
    # the record that passes start + 16666 closes the group and is part of it
    assert _scan([5, 10, 2 + V]) == (0, 0, 2, 2 + V)
    assert _scan([5, 10, 3 + V, 7]) == (3, 1, 3 + V, 3 + V)
    # the next group starts at running_t, which counts records that close nothing
    assert _scan([3 + V, 100 + V, 3 + 2 * V, 101 + 2 * V]) == (4, 2, 101 + 2 * V, 101 + 2 * V)
    # out-of-order t: running_t is a max
    assert _scan([50000, 10, 60000]) == (1, 1, 50000, 60000)
    # the dropped last group still counts in running_t
    assert _scan([V + 3, V + 5, V + 9]) == (1, 1, V + 3, V + 9)
    # u32 wrap near 2^32: start + 16666 wraps, so any t above the wrapped limit closes the group
    top = (1 << 32) - 100
    assert _scan([10, 20000], top, top) == (2, 1, top, top)  # limit = 16566
    assert _scan([16566, 16567, 5], top, top) == (2, 1, top, top)
    # splits: scanning in pieces carries the state
    ts = [random.Random(5).randrange(0, 200000) for _ in range(3000)]
    done, g, s, rt = _scan(ts)
    d1, g1, s1, rt1 = _scan(ts[:1234])
    d2, g2, s2, rt2 = _scan(ts[1234:], s1, rt1)
    assert (s2, rt2, g1 + g2) == (s, rt, g) and (d2 + 1234 if d2 else d1) == done


def test_group_scan_equals_the_oracle():
    rng = np.random.default_rng(2)
    ts = np.sort(rng.integers(0, 400000, 2000)).tolist()
    ts[100:110] = [5] * 10  # late records
    # the oracle's reading loop
    start, rt, done = 2, 2, 0
    for i, t in enumerate(ts):
        rt = max(rt, t)
        if t > ((start + R.VIEW_INTERVAL) & R.M32):
            done, start = i + 1, rt
    got = _scan(ts)
    assert (got[0], got[2], got[3]) == (done, start, rt)


def _chain(recs, W, H, ref_time=1):
    """The oracle's per-record steps (no integration)."""
    src = R.Prophesee.__new__(R.Prophesee)
    src.W, src.H, src.ref_time, src.theta = W, H, ref_time, 0.02
    src.last_t, src.last_ln = [2] * (W * H), [LN_MID] * (W * H)
    steps = []

    class V:
        def integrate_sparse(self, s):
            steps.extend(s.tolist())
            return np.zeros(0)
    src.v = V()
    src.consume_batch([(i, *r) for i, r in enumerate(recs)])
    return steps, src


def test_chain_hand_cases():
    # t == last_t: ln moves, no step; t < last_t: skipped; t > last_t + 1: the gap step first
    steps, src = _chain([(2, 0, 0, 1), (1, 0, 0, 1), (5, 0, 0, 0), (5, 0, 0, 0)], 1, 1, ref_time=20)
    ln1 = LN_MID + 0.02
    v_gap = (P.exp(ln1) - 1.0) * 255.0
    ln2 = ln1 - 0.02
    v2 = (P.exp(ln2) - 1.0) * 255.0
    assert len(steps) == 2
    assert steps[0][3] == int(v_gap) and steps[0][4] == 1 and steps[0][6] == np.float32(2 * 20)
    assert steps[0][5] == np.float32(v_gap * 2.0)
    assert steps[1][3] == int(v2) and steps[1][4] == 0 and steps[1][6] == np.float32(20)
    assert src.last_t[0] == 5 and src.last_ln[0] == ln2 - 0.02
    # the clamp: a bright pixel past 255 comes back to 128 and ln_1p(128 / 255)
    recs = [(2, 0, 0, 1)] * 40 + [(3, 0, 0, 1)]
    steps, src = _chain(recs, 1, 1)
    assert steps[-1][3] == 128 and src.last_ln[0] == LN_MID


def test_end_assert():
    # the only record of the last complete group has the largest t: its pixel's last t == running_t
    V = R.VIEW_INTERVAL
    recs = [(3 + V, 0, 0, 1)]
    assert _scan([3 + V]) == (1, 1, 3 + V, 3 + V)
    src = R.Prophesee(2, 1, 1)
    with pytest.raises(R.EndAssert):
        src.run(recs)
    # a later record in the dropped group moves running_t past it: no assert
    assert _scan([3 + V, 4 + V])[3] == 4 + V
    R.Prophesee(2, 1, 1).run([(3 + V, 0, 0, 1), (4 + V, 1, 0, 0)])
