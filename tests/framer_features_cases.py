"""Hand-derived known answers for feature detection while framing, one per rule of Framer::ingest_event
(driver.rs:446-553) -- test helper shared by the CPU and the GPU suite.

A case is a list of operations run against any implementation (the Python restatement, the C++ mirror, the device
logic compiled for the host, the device) through `run`, and what must come out: the features of every ingest call
as (index, t, x, y), and the intervals of every pop_features as (end_ts, [(x, y)]) or "broken".

All cases: tps 7650, ref_interval 255, output_fps 30 -> tpf 255; framed source, so a pixel's clock is rounded up to a
multiple of 255 after every event.  Intensities used: (d 7, t 255) -> 128, (d 0, t >= 200) -> 1 or 0, (d 7, t 136) -> 240
or 239, (d 10, t 255) -> 1024 in a u16 frame.  On the 9 x 9 plane only (3..5, 3..5) is 3 pixels off the border; the ring
of (4, 4) lies on the border entirely, so ring events are never features themselves.
"""
import numpy as np

from framer_features_oracle import make_events, DELTA_T, ABSOLUTE_T, DequeBroken

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]  # cv.rs:25-30 (dx, dy)

BASE = dict(width=9, height=9, channels=1, tps=7650, ref_interval=255, delta_t_max=7650, output_fps=30.0,
            codec_version=2, time_mode=DELTA_T)
ABS = dict(BASE, time_mode=ABSOLUTE_T)


def ring(cx, cy, d, t, c=None, only=None):
    return [(cx + dx, cy + dy, c, d, t) for k, (dx, dy) in enumerate(RING) if only is None or k in only]


def case(name, params, ops, features, pops=()):
    return dict(name=name, params=params, ops=ops, features=[list(f) for f in features], pops=list(pops))


DUMMY = (0, 0, None, 7, 100)  # a border event that only provides a last_event

CASES = [
    # the plane is prepared (ring 128), then last_event = None: the centre (value 1) is not looked at
    case("first_event_of_a_stream_is_never_tested", BASE,
         [("detect", True), ("ingest", ring(4, 4, 7, 255)), ("reset",), ("ingest", [(4, 4, None, 0, 200)])],
         [[], []]),
    # the same without the reset: last.t = 255 != 200, ring 128 > 1 + 30 all round
    case("carried_last_event_makes_it_a_candidate", BASE,
         [("detect", True), ("ingest", ring(4, 4, 7, 255)), ("ingest", [(4, 4, None, 0, 200)])],
         [[], [(0, 200, 4, 4)]]),
    case("same_t_as_the_previous_event_is_not_tested", BASE,
         [("detect", True), ("ingest", ring(4, 4, 7, 255) + [(4, 4, None, 0, 255)])],
         [[]]),
    # AbsoluteT: (0, 0) fires at 300 (clock -> 510) and at 700, which crosses a frame: event.t becomes 700 - 510 = 190.
    # The centre at raw t 700 equals the previous RAW t, and is tested only because last.t is 190
    case("absolute_t_overwritten_last_t_makes_a_pair_tested", ABS,
         [("detect", True), ("ingest", ring(4, 4, 7, 255) + [(0, 0, None, 7, 300), (0, 0, None, 7, 700),
                                                             (4, 4, None, 0, 700)])],
         [[(18, 700, 4, 4)]]),
    # ... and the centre at t 190 differs from the previous raw t, and is skipped only because last.t is 190
    case("absolute_t_overwritten_last_t_makes_a_pair_skipped", ABS,
         [("detect", True), ("ingest", ring(4, 4, 7, 255) + [(0, 0, None, 7, 300), (0, 0, None, 7, 700),
                                                             (4, 4, None, 0, 190)])],
         [[]]),
    # three channels: bright ring on channel 1 only (the ring reads channel 0: zeros); the centre on channel 1 is never
    # tested; the centre on channel 0 (128) sees a dark ring (0 < 98)
    case("only_channel_0_is_tested_and_the_ring_reads_channel_0", dict(BASE, channels=3),
         [("detect", True), ("ingest", ring(4, 4, 7, 255, c=1) + [(4, 4, 1, 0, 200), (4, 4, 0, 7, 255)])],
         [[(17, 255, 4, 4)]]),
    # a bright pixel (128) over zeros is a corner wherever it may be one: x = 2 and x = 6 are within 3 of the border
    case("three_pixel_border_rejects", BASE,
         [("detect", True), ("ingest", [DUMMY, (2, 4, None, 7, 255), (3, 4, None, 7, 254), (6, 4, None, 7, 255),
                                        (4, 2, None, 7, 254), (4, 6, None, 7, 255), (5, 5, None, 7, 254)])],
         [[(2, 254, 3, 4), (6, 254, 5, 5)]]),
    # the same multiset in two orders: ring first, the centre (1) sees 128s; centre first, it sees zeros
    case("ring_events_before_the_candidate_count", BASE,
         [("detect", True), ("ingest", [DUMMY] + ring(4, 4, 7, 255) + [(4, 4, None, 0, 200)])],
         [[(17, 200, 4, 4)]]),
    case("ring_events_after_the_candidate_do_not_count", BASE,
         [("detect", True), ("ingest", [DUMMY, (4, 4, None, 0, 200)] + ring(4, 4, 7, 255))],
         [[]]),
    # u16 frames of a U16 source: the centre's intensity is 1024, `as u8` gives 255 (not 1024 & 255 = 0).  A ring of
    # 240 is then neither darker than 225 nor (as it would be over 0) brighter than 30 ...
    case("as_u8_saturates_u16_frames_ring_240", dict(BASE, value_type=1, source_type=1),
         [("detect", True), ("ingest", [DUMMY] + ring(4, 4, 7, 136) + [(4, 4, None, 10, 255)])],
         [[]]),
    # ... and a ring of 128 is darker than 225
    case("as_u8_saturates_u16_frames_ring_128", dict(BASE, value_type=1, source_type=1),
         [("detect", True), ("ingest", [DUMMY] + ring(4, 4, 7, 255) + [(4, 4, None, 10, 254)])],
         [[(17, 254, 4, 4)]]),
    # the centre gets 128 while detection is off (plane stays 0); a D_EMPTY event then crosses a frame, keeps 128,
    # WRITES it and is tested: 128 over zeros.  Were the plane not written the centre would read 0: no corner
    case("d_empty_event_writes_the_plane_and_is_a_candidate", BASE,
         [("ingest", [(4, 4, None, 7, 255)]), ("detect", True), ("ingest", [DUMMY, (4, 4, None, 255, 300)])],
         [[], [(1, 300, 4, 4)]]),
    # AbsoluteT: the centre fires at 600 (value 54, clock -> 765) with detection off; an event at 300 lies in its past:
    # the trackers stay, the plane gets 54 and the event is tested (zeros are darker than 24)
    case("absolute_t_event_from_the_past_writes_and_tests", ABS,
         [("ingest", [(4, 4, None, 7, 600)]), ("detect", True), ("ingest", [DUMMY, (4, 4, None, 7, 300)])],
         [[], [(1, 300, 4, 4)]]),
    # eight alternate ring pixels of (3, 3) are written 128 with detection on, then set to 1 with detection off: the plane
    # keeps 128.  The centre (128) sees dark arcs of length 1 only; a fresh plane would give an all-dark ring
    case("plane_is_stale_after_detection_was_off", BASE,
         [("detect", True), ("ingest", [DUMMY] + ring(3, 3, 7, 255, only=range(0, 16, 2))),
          ("detect", False), ("ingest", ring(3, 3, 0, 255, only=range(0, 16, 2))),
          ("detect", True), ("ingest", [DUMMY, (3, 3, None, 7, 255)])],
         [[], [], []]),
    # deque, first feature: time 200, frames_written 0 -> idx 0; the deque is created as [255, 510], nothing grows
    case("deque_first_feature", BASE,
         [("detect", True), ("ingest", [DUMMY, (4, 4, None, 7, 200)]), ("pop_features", 3)],
         [[(1, 200, 4, 4)]], [(255, [(4, 4)]), (510, []), (765, [])]),
    # growth: time 2000 (d 12: 255 after saturation) -> idx 7; [255, 510] grows by 765 .. 2040 (six intervals)
    case("deque_grows_across_empty_intervals", BASE,
         [("detect", True), ("ingest", [DUMMY, (4, 4, None, 12, 2000)]), ("pop_features", 9)],
         [[(1, 2000, 4, 4)]],
         [(255 * (k + 1), []) for k in range(7)] + [(2040, [(4, 4)]), (2295, [])]),
    # three frames are framed and popped with detection off (every pixel: d 7, t 765 -> 42 in frames 0..2), then a feature
    # at time 1000: idx = 1000 / 255 - 3 = 0, the deque is created as [255, 510] and interval 0's end is raised to 1000
    case("deque_end_ts_raised_when_detection_is_switched_on_late", BASE,
         [("ingest", [(x, y, None, 7, 765) for y in range(9) for x in range(9)]), ("pop", 3), ("detect", True),
          ("ingest", [DUMMY, (4, 4, None, 12, 1000)]), ("pop_features", 2)],
         [[], [(1, 1000, 4, 4)]], [(1000, [(4, 4)]), (510, [])]),
    case("pop_features_on_an_empty_deque", BASE,
         [("detect", True), ("pop_features", 3)],
         [], [(255, []), (510, []), (765, [])]),
    # two pops leave [765]; a feature at 300 wants idx 1, nothing grows (765 + 255 > 510): the reference panics
    case("feature_past_the_deque_is_reported", BASE,
         [("detect", True), ("pop_features", 2), ("ingest", [DUMMY, (4, 4, None, 7, 300)]), ("pop_features", 1)],
         [[(1, 300, 4, 4)]], [(255, []), (510, []), "broken"]),
]


def run(impl, ops):
    """impl: detect_features(on), reset_last_event(), ingest(events) -> FEATURE_DTYPE array, pop() -> bytes,
    write_frame_bytes() -> bytes,
    pop_features() -> (end_ts, [n][2]) or raises DequeBroken, running_intensities() -> [h][w][c] u8."""
    log = dict(features=[], pops=[], frames=[])
    for op in ops:
        if op[0] == "detect":
            impl.detect_features(op[1])
        elif op[0] == "reset":
            impl.reset_last_event()
        elif op[0] == "ingest":
            f = impl.ingest(op[1] if isinstance(op[1], np.ndarray) else make_events(op[1]))
            log["features"].append([(int(r["index"]), int(r["t"]), int(r["x"]), int(r["y"])) for r in f])
        elif op[0] == "pop":
            frames = impl.pop()
            if op[1] is not None:
                assert len(frames) == op[1] * len(np.asarray(impl.running_intensities()).ravel()) * impl_bytes(impl)
            log["frames"].append(frames)
        elif op[0] == "pop_with_features":  # the player: one FeatureInterval per frame it takes
            frames = impl.pop()
            log["frames"].append(frames)
            for _ in range(len(frames) // (np.asarray(impl.running_intensities()).size * impl_bytes(impl))):
                end_ts, xy = impl.pop_features()
                log["pops"].append((int(end_ts), [tuple(int(v) for v in p) for p in np.asarray(xy).reshape(-1, 2)]))
        elif op[0] == "write_frame":  # write_frame_bytes: frame 0 as it is, complete or not
            for _ in range(op[1]):
                log["frames"].append(impl.write_frame_bytes())
        elif op[0] == "pop_features":
            for _ in range(op[1]):
                try:
                    end_ts, xy = impl.pop_features()
                    log["pops"].append((int(end_ts), [tuple(int(v) for v in p) for p in np.asarray(xy).reshape(-1, 2)]))
                except DequeBroken:
                    log["pops"].append("broken")
    log["plane"] = np.asarray(impl.running_intensities()).copy()
    return log


def impl_bytes(impl):
    return 1 << getattr(impl, "value_type_log2", 0)
