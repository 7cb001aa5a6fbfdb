"""Streams for the DVS event video (include/adder_dvs.h), seeded or hand-built, a few hundred to a few thousand events
each, with the census every one must reach (tests/dvs_video_oracle.py counts it): tests/test_dvs_video_cpu.py asserts
it, so a case that stops reaching its arm fails.  tests/test_gpu_dvs_video.py runs every case on the device.

A case: dict(name, meta, tps, fps, buffer_secs, draw, ring, events, census) -- census maps a counter to the least
count the oracle must report (0: exactly 0).  `ring`: ring frames for a whole-stream call.
"""
import numpy as np

import adder_stream_np as S
from test_dvs_cpu import DVS_CAM, GOLDENS, golden_bytes

NONE = 0xFF
D_SET = np.array([0, 1, 2, 3, 5, 7, 8, 9, 12, 20, 40, 127, 128, 255], np.uint8)


def meta_of(w, h, ch=1, time_mode=0, ref=255, cam=0):
    return dict(width=w, height=h, channels=ch, time_mode=time_mode, ref_interval=ref, source_camera=cam)


def events_of(rows):
    """rows of (x, y, c, d, t)"""
    ev = np.zeros(len(rows), S.EVENT_DTYPE)
    for k, name in enumerate(("x", "y", "c", "d", "t")):
        ev[name] = [r[k] for r in rows]
    return ev


def seeded(seed, n, w, h, ch, time_mode, dt_max=600, jump=0.0, jump_len=40_000):
    """Every unit's times ascend.  DeltaT: t is the step; AbsoluteT: t is the unit's time.  jump: the share of events
    whose step is about jump_len ticks (a long quiet gap for that unit, and for the stream when it leads)."""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, S.EVENT_DTYPE)
    ev["x"] = rng.integers(0, w, n)
    ev["y"] = rng.integers(0, h, n)
    ev["c"] = rng.integers(0, ch, n) if ch > 1 else NONE
    ev["d"] = rng.choice(D_SET, n)
    step = rng.integers(0, dt_max, n)
    step = np.where(rng.random(n) < jump, jump_len + rng.integers(0, 999, n), step)
    last = {}
    for i in range(n):
        u = (int(ev["x"][i]), int(ev["y"][i]), int(ev["c"][i]))
        if u not in last and ev["d"][i] == 255:
            ev["d"][i] = 6  # a unit's first event has d <= 128
        t = last.get(u, 0) + int(step[i])
        last[u] = t
        ev["t"][i] = int(step[i]) if time_mode == 0 else t
    return ev


def case(name, meta, stream, tps=25500, fps=100.0, buffer_secs=0.02, draw=True, ring=4096, golden=None, **census):
    return dict(name=name, meta=meta, tps=tps, fps=fps, buffer_secs=buffer_secs, draw=draw, ring=ring,
                events=stream, golden=golden, census=census)


def slow_unit():
    """unit 0 leads with steps of 1000 ticks, unit 1 crawls with steps of 10: its old_t + 1 lies in frames popped long
    ago, so its fires reach the DVS output and are dropped from the video"""
    rows = [(0, 0, NONE, 5, 1000), (1, 0, NONE, 5, 10)]
    for k in range(300):
        rows.append((0, 0, NONE, 3 + k % 5, 1000))
        rows.append((1, 0, NONE, 3 + (k + 2) % 5, 10))
    return events_of(rows)


def quiet_gap_then_restart():
    """L = 255, B = 510.  Unit 0 jumps 100 frames ahead; 150 events that fire nothing (d = 255, step 0) let the pops
    run the deque dry and skip indices; then unit 0 fires again: the deque restarts at frame_count"""
    rows = [(0, 0, NONE, 5, 300), (1, 0, NONE, 5, 300), (0, 0, NONE, 7, 300), (0, 0, NONE, 5, 255 * 100)]
    rows += [(1, 0, NONE, 255, 0)] * 150
    rows += [(0, 0, NONE, 7, 100), (0, 0, NONE, 5, 100), (1, 0, NONE, 7, 255 * 101), (1, 0, NONE, 5, 50)]
    return events_of(rows)


def empty_at_finish():
    """as above, but the stream ends while the deque is empty: finish emits one blank frame"""
    rows = [(0, 0, NONE, 5, 300), (0, 0, NONE, 7, 300), (0, 0, NONE, 5, 255 * 20)]
    rows += [(1, 0, NONE, 5, 0)] + [(1, 0, NONE, 255, 0)] * 60
    return events_of(rows)


def same_pixel():
    """two fires of opposite polarity on pixel (1, 2) inside one frame (the later one wins), and fires from channels
    0 and 2 of pixel (3, 1) into one frame"""
    rows = [(2, 1, 0, 5, 100), (2, 1, 0, 9, 10), (2, 1, 0, 3, 10),  # up, then down: frame 0 both
            (1, 3, 0, 5, 100), (1, 3, 2, 5, 100), (1, 3, 0, 9, 20), (1, 3, 2, 2, 20)]  # c0 up, c2 down
    return events_of(rows)


def far_ahead():
    """unit 0's third event fires at old_t + 1 = 1000 frames ahead of frame_count: 1001 ring slots in one call"""
    rows = [(0, 0, NONE, 5, 10), (0, 0, NONE, 7, 255 * 1000), (0, 0, NONE, 5, 1), (1, 0, NONE, 5, 10)]
    return events_of(rows)


def bad_middle():
    ev = seeded(31, 600, 5, 4, 1, 0)
    ev["d"][300] = 200  # d in 129..254
    return ev


def wrap_counts():
    """unit (0, 0) gets 65 539 events: the reference's u16 counter wraps to 3 and its maximum stays 65535"""
    n = 65_539
    ev = np.zeros(n + 40, S.EVENT_DTYPE)
    ev["c"] = NONE
    ev["d"] = 255
    ev["d"][0] = 5
    ev["t"][0] = 7
    tail = seeded(5, 40, 5, 4, 1, 0)
    tail["x"] = np.maximum(tail["x"], 1)  # not unit (0, 0)
    ev[n:] = tail
    return ev


def synthetic_cases():
    cs = []
    k = 0
    for (w, h) in ((5, 4), (33, 3), (67, 5)):
        for ch in (1, 3):
            for time_mode in (0, 1):
                cam, ref = ((0, 255), (DVS_CAM, 5000), (0, 5000), (DVS_CAM, 255))[k % 4]
                k += 1
                n = 1500 if w * h * ch < 200 else 3000
                cs.append(case(f"seeded_{w}x{h}x{ch}_tm{time_mode}_cam{cam}_ref{ref}", meta_of(w, h, ch, time_mode, ref, cam),
                               seeded(100 + k, n, w, h, ch, time_mode, jump=0.002, jump_len=12_000), buffer_secs=0.2,
                               fired=100, late=1, drawn=10))
    cs.append(case("seeded_130x66", meta_of(130, 66, 1, 0, 255, 0), seeded(7, 4000, 130, 66, 1, 0, dt_max=3000),
                   buffer_secs=0.15, fired=100, drawn=20, pops=3))
    cs.append(case("nothing_pops", meta_of(5, 4), seeded(3, 200, 5, 4, 1, 0, dt_max=20), buffer_secs=10.0,
                   fired=20, pops=0))
    cs.append(case("quiet_gap_then_restart", meta_of(5, 4, cam=DVS_CAM), quiet_gap_then_restart(),
                   empty_pops=50, restarts=1, skipped=50))
    cs.append(case("empty_at_finish", meta_of(5, 4, cam=DVS_CAM), empty_at_finish(), empty_pops=1, blank_at_finish=1))
    cs.append(case("slow_unit", meta_of(5, 4, cam=DVS_CAM), slow_unit(), buffer_secs=0.0, late=200, fired=400))
    cs.append(case("same_pixel", meta_of(5, 4, 3, cam=DVS_CAM), same_pixel(), overwritten=2, fired=4))
    cs.append(case("far_ahead", meta_of(5, 4, cam=DVS_CAM), far_ahead(), ring=1001, fired=2))
    cs.append(case("b0_l1", meta_of(5, 4, cam=DVS_CAM), seeded(9, 800, 5, 4, 1, 0, dt_max=4), tps=100, fps=100.0,
                   buffer_secs=0.0, fired=100, late=1))
    # 25500 / 29.97f: 850.85 in f32 and f64 alike; 3 / 0.3f is 10 in f32 (9.9999996 rounds up) and 9 in f64
    cs.append(case("f32_truncation", meta_of(5, 4, cam=DVS_CAM), seeded(12, 800, 5, 4, 1, 0, dt_max=40), tps=3,
                   fps=0.3, buffer_secs=1.0, fired=100))
    cs.append(case("fractional_fps", meta_of(33, 3, 3, 1, 255, 0), seeded(13, 1500, 33, 3, 3, 1), fps=29.97,
                   fired=100))
    cs.append(case("draw_off_two_blanks", meta_of(5, 4), seeded(14, 600, 5, 4, 1, 0), draw=False, fired=100))
    cs.append(case("draw_off_one_blank", meta_of(5, 4), seeded(3, 200, 5, 4, 1, 0, dt_max=20), buffer_secs=10.0,
                   draw=False, fired=20))
    cs.append(case("bad_middle", meta_of(5, 4), bad_middle(), fired=50))
    cs.append(case("wrap_counts", meta_of(5, 4, cam=DVS_CAM), wrap_counts(), buffer_secs=10.0, events=65_579))
    return cs


def golden_cases():
    cs = []
    for name in GOLDENS:
        buf = golden_bytes(name)
        meta, ev, _ = S.read_adder(buf)
        m = {k: meta[k] for k in ("width", "height", "channels", "time_mode", "ref_interval", "source_camera")}
        cs.append(case(f"{name}_cli_defaults", m, ev, tps=meta["tps"], fps=100.0, buffer_secs=10.0, ring=0, golden=name))
        cs.append(case(f"{name}_fps1000", m, ev, tps=meta["tps"], fps=1000.0, buffer_secs=0.001, ring=0, golden=name))
    return cs
