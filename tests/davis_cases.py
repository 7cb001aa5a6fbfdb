"""Constructed DAVIS packets for the chain's tests: each case is a few packets on a small plane, built so that one
part of the chain meets its edges.  A case is a dict(name, W, H, mode, tps, ref_time, dtm, crf, packets); a packet is a
dict(frame [H, W] f64, c, start, end, before, after).  seeded(mode) rebuilds the packets of
test_host_mirror.test_davis_source_frames_and_dvs_events_interleaved."""
import numpy as np

from davis_oracle import EVENT_DTYPE, FRAMED, RAW_DAVIS, RAW_DVS, events

TPS, REF, DTM = 1_000_000, 5000, 500_000


def seeded(mode):
    """The 38x28x7 packets of the mirror's test, from the same generator calls in the same order."""
    rng = np.random.default_rng(20 + mode)
    W, H, P = 38, 28, 7
    packets, t = [], 40_000
    base = rng.random((H, W))
    for k in range(P):
        start, end = t, t + int(rng.integers(3000, 9000))
        nxt = end + int(rng.integers(10_000, 30_000))

        def evs(lo, hi, n):
            ev = np.zeros(n, EVENT_DTYPE)
            ev["t"] = np.sort(rng.integers(lo, hi, n))
            hot = rng.integers(0, W * H, 25)
            pix = np.where(rng.random(n) < 0.6, hot[rng.integers(0, 25, n)], rng.integers(0, W * H, n))
            ev["x"], ev["y"], ev["on"] = pix % W, pix // W, rng.integers(0, 2, n)
            return ev
        frame = np.clip(base + rng.normal(0, 0.08, (H, W)) + (0.3 if k == 4 else 0.0), -0.05, 1.1)
        packets.append({"frame": frame, "c": 0.1 + 0.05 * rng.random(), "start": start, "end": end,
                        "before": evs(start - 25_000, start + 2000, 400), "after": evs(end - 2000, nxt + 1000, 400)})
        t = nxt
    return dict(name=f"seeded_mode{mode}", W=W, H=H, mode=mode, tps=TPS, ref_time=REF, dtm=DTM,
                crf=2 if mode else None, packets=packets)


def _random_events(rng, W, H, n, lo, hi, hot=None):
    t = np.sort(rng.integers(lo, max(hi, lo + 1), n))
    pix = rng.integers(0, W * H, n)
    if hot is not None and n:
        pix = np.where(rng.random(n) < 0.6, hot[rng.integers(0, len(hot), n)], pix)
    return events(t, pix % W, pix // W, rng.integers(0, 2, n))


def _packets(rng, W, H, P, n_before, n_after, *, t0=40_000, gap=20_000, exposure=5000, frame=None, c=None, hot=None):
    """P packets `gap` apart; before events from the previous end to a little past the start, after events from a little
    before the end to a little past the next start, so that every check has events on both sides."""
    out, start = [], t0
    for k in range(P):
        end, nxt = start + exposure, start + exposure + gap
        nb = n_before[k] if isinstance(n_before, (list, tuple)) else n_before
        na = n_after[k] if isinstance(n_after, (list, tuple)) else n_after
        fr = frame(k) if frame else np.clip(rng.random((H, W)), 0.02, 0.98)
        out.append({"frame": np.asarray(fr, np.float64).reshape(H, W), "c": c(k) if c else 0.15, "start": start, "end": end,
                    "before": _random_events(rng, W, H, nb, start - gap, start + gap // 10, hot),
                    "after": _random_events(rng, W, H, na, end - gap // 10, nxt + gap // 10, hot)})
        start = nxt
    return out


def _case(name, W, H, mode, packets, *, tps=TPS, ref_time=REF, dtm=DTM, crf=None):
    return dict(name=name, W=W, H=H, mode=mode, tps=tps, ref_time=ref_time, dtm=dtm, crf=crf, packets=packets)


def _order_case():
    # arrival order walks the chunks 3, 0, 2, 1 and comes back to the same pixels, pixel index falling inside a
    # chunk: chunk-major order, arrival order and pixel order all differ
    W, H = 38, 28
    rng = np.random.default_rng(101)
    packets = _packets(rng, W, H, 3, 0, 0)
    for k, pk in enumerate(packets):
        for name, lo, hi in (("before", pk["start"] - 15_000, pk["start"]), ("after", pk["end"] + 1, pk["end"] + 15_000)):
            n = 240
            ys = np.array([(27 - i % 7, i % 7, 20 - i % 7, 13 - i % 7)[i % 4] for i in range(n)])
            xs = (37 - (np.arange(n) * 5) % 38) % 38
            xs[::3] = 11  # pixels that come back
            t = np.linspace(lo, hi - 1, n).astype(np.int64)
            pk[name] = events(t, xs, ys, (np.arange(n) + k) % 3 != 0)
    return _case("order", W, H, RAW_DAVIS, packets, crf=2)


def _rawdvs_case():
    # RawDvs has no second check: `after` events before the previous end (= previous start + 1) reach the
    # negative-ticks arm
    W, H = 38, 28
    rng = np.random.default_rng(102)
    packets = _packets(rng, W, H, 4, 150, 150, hot=rng.integers(0, W * H, 9))
    for pk in packets:
        n = 40
        pix = rng.integers(0, W * H, n)
        early = events(np.sort(rng.integers(pk["start"] - 3000, pk["start"] + 1, n)), pix % W, pix // W,
                       rng.integers(0, 2, n))
        pk["after"] = np.concatenate([early, pk["after"]])
    return _case("rawdvs_after_before_end", W, H, RAW_DVS, packets, crf=1)


def _first_packet_case():
    W, H = 4, 4
    rng = np.random.default_rng(103)
    packets = _packets(rng, W, H, 2, 60, 30)
    packets[0]["before"] = _random_events(rng, W, H, 60, 1000, packets[0]["start"])  # all pass the check, last_ts is 0
    packets[0]["after"]["t"][:2] = packets[0]["end"], packets[0]["end"] + 1  # on the second check's edge, and one past
    return _case("first_packet", W, H, RAW_DAVIS, packets)


def _high_clamp_case():
    W, H = 38, 28
    rng = np.random.default_rng(104)
    packets = _packets(rng, W, H, 3, 0, 0, c=lambda k: 1.5, frame=lambda k: np.full((H, W), 0.55 + 0.1 * k))
    for pk in packets:
        for name, lo in (("before", pk["start"] - 9000), ("after", pk["end"] + 10)):
            n = 120
            pix = np.repeat(np.array([5, 5 + 38 * 9, 500, 1063]), n // 4)
            t = lo + np.arange(n) * 60
            pk[name] = events(t, pix % W, pix // W, (np.arange(n) % 10) != 9)  # runs of on events, an off now and then
    return _case("high_clamp", W, H, RAW_DAVIS, packets, crf=3)


def _gap_low_clamp_case(W, H):
    # frames of 0.0, of negative values above -1 and of values above 1; packet 2 starts where packet 1 ended (no ticks
    # in its gaps); events on the clamped pixels
    rng = np.random.default_rng(105 + W)
    vals = np.array([0.0, -0.05, -0.9, 1.3, 2.0, 0.4, 1.0, 0.999])

    def frame(k):
        return vals[(np.arange(W * H) + k) % len(vals)].reshape(H, W)
    packets = _packets(rng, W, H, 4, 70, 70, frame=frame)
    shift = packets[2]["start"] - packets[1]["end"]
    for pk in packets[2:]:
        pk["start"] -= shift
        pk["end"] -= shift
        for name in ("before", "after"):
            pk[name]["t"] -= shift
    return _case(f"gap_low_clamp_{W}x{H}", W, H, RAW_DAVIS, packets, crf=0)


def tie_down_value():
    """A frame value whose product with 255.0 is exactly k + 0.5 with k even: found by search."""
    for k in range(2, 254, 2):
        v = (k + 0.5) / 255.0
        for cand in (v, np.nextafter(v, 0.0), np.nextafter(v, 1.0)):
            if float(cand) * 255.0 == k + 0.5:
                return float(cand), k
    raise AssertionError("no tie-down value")


def _rounding_case(mode):
    W, H = 38, 28
    rng = np.random.default_rng(106)
    v, _ = tie_down_value()

    def frame(k):
        f = np.clip(rng.random((H, W)), 0.02, 0.98)
        f.flat[::5] = 0.5   # 127.5: tie to 128
        f.flat[1::5] = v    # k + 0.5, k even: tie to k
        f.flat[2::97] = 1.5
        f.flat[3::97] = -0.25
        return f
    return _case(f"rounding_mode{mode}", W, H, mode, _packets(rng, W, H, 2, 50, 50, frame=frame), crf=2 if mode else None)


def _long_run_case():
    # one pixel with 3000 events in one list: a run longer than any block
    W, H = 1, 8
    rng = np.random.default_rng(107)
    packets = _packets(rng, W, H, 2, 20, 20, gap=200_000)
    pk = packets[1]
    n = 3000
    pk["before"] = events(pk["start"] - 190_000 + np.arange(n) * 60, np.zeros(n), np.full(n, 5), rng.integers(0, 2, n))
    return _case("long_run", W, H, RAW_DAVIS, packets, crf=2)


def _count_case():
    W, H = 300, 8
    rng = np.random.default_rng(108)
    nb, na = [0, 1, 255, 256, 257, 1025], [1025, 257, 256, 255, 1, 0]
    return _case("counts", W, H, RAW_DAVIS, _packets(rng, W, H, 6, nb, na, hot=rng.integers(0, W * H, 5)), crf=2)


def _time_case(bits, mode, tps):
    # the second packet starts 2^bits us after the first: (f32)dmicro is inexact, and 32-bit time would wrap
    W, H = 4, 4
    rng = np.random.default_rng(109 + bits)
    packets = _packets(rng, W, H, 3, 50, 50)
    shift = (1 << bits) + 12_345
    for pk in packets[1:]:
        pk["start"] += shift
        pk["end"] += shift
        for name in ("before", "after"):
            pk[name]["t"] += shift
    late = packets[0]["after"].copy()  # the first packet's late `after` events follow the shift
    late["t"][len(late) // 2:] += shift
    packets[0]["after"] = late
    return _case(f"time_2p{bits}_mode{mode}", W, H, mode, packets, tps=tps, crf=2)


def build():
    return [_order_case(), _rawdvs_case(), _first_packet_case(), _high_clamp_case(), _gap_low_clamp_case(4, 4),
            _gap_low_clamp_case(38, 28), _rounding_case(RAW_DAVIS), _rounding_case(FRAMED), _long_run_case(), _count_case(),
            _time_case(24, RAW_DAVIS, 1_000_000), _time_case(31, RAW_DVS, 50_000), _time_case(40, RAW_DAVIS, 100)]


def _list_cases():
    """integrate_dvs_events called on its own with the second check in its other form (t < ts2), which no consume()
    path takes: dict(name, W, H, last_ts, last_ln, events, ts1, ts2, after2, c, tps, ref_time)."""
    out = []
    for W, H, seed in ((6, 8, 5), (38, 28, 6)):
        rng = np.random.default_rng(seed)
        out.append(dict(name=f"before_form_{W}x{H}", W=W, H=H, last_ts=np.full(W * H, 500, np.int64),
                        last_ln=np.log1p(rng.random(W * H)), events=_random_events(rng, W, H, 300, 1000, 9000), ts1=8000,
                        ts2=4000, after2=False, c=0.2, tps=TPS, ref_time=REF))
    return out


CASES = build()
LIST_CASES = _list_cases()
SEEDED = [seeded(m) for m in (FRAMED, RAW_DAVIS, RAW_DVS)]
