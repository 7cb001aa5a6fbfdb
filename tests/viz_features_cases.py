"""Hand-derived known answers for feature detection in the adder-viz player, one per rule of
include/adder_viz_player.h ("Feature detection") -- test helper shared by the CPU and the GPU suite.

The 9 x 9 plane of tests/framer_features_cases.py (its `ring`, DUMMY-style border events and intensities): tps 7650,
ref_interval 255, 30 fps -> tpf 255, framed source (a unit's clock is rounded up to a multiple of 255 after every event),
buffer_limit 1.  Intensities: (d 7, t 255) -> 128, (d 7, t 765) -> 42, (d 7, t 510) -> 64, (d 7, t 1000) -> 32,
(d 7, t 100) -> 255 (saturated), (d 0, t 200) -> 1, (d 0, t 600) -> 0.  Only (3..5, 3..5) is 3 pixels off the border.

Building blocks.  FULL: every unit fires (d 7, t 255): frame 0 is complete at its last event (P = 80) and all 128; all
its t are equal, so none of its events is tested.  JUMPS(rows): (0, y) fires (d 7, t 765): last_filled 3 >
frames_written 1 + limit 1, the row is forced; when every row is forced frame 1 is popped, and frame 2 right after it
(the deque still holds 2 > limit frames).  Column 0 and (8, 0) lie on no FAST ring of (4, 4); the ring of (3, 3) holds
(0, 2), (0, 3), (0, 4), which are still 128 when (3, 3) fires.

The interval deque runs from creation: the pop of frame j takes the interval that ends at 255 * (j + 1).

A case is a list of operations run against any implementation through `run`, and per ingest / finish call what must
come out: features (index, t, x, y), pops P_j, intervals (end_ts, [(x, y)]), and -- where the rule is about frames --
both frame forms.  `None` = not hand-derived here (the GPU suite still compares it with the restatement).

The deque the reference would panic over is reached where (time / tpf + 1) * tpf wraps u32 while the unit stays inside
the frame ring (tpf > 2^32 / ring_frames): `a_feature_past_the_deque_is_reported_while_frames_go_on`, at tpf 2^17 and a
ring of 65536 frames.  Two rules cannot be reached through the player and have no case: growth of the deque by 2^22
intervals (the unit would be 2^22 frames ahead of a ring of at most 65536: refused) and the raised end_ts of
driver.rs:544-547: every pop takes an interval, so the front of the deque always ends at (frames_written + 1) * tpf, and
interval idx = time / tpf - frames_written (or 0) then ends at or after `time`.  `detection_switched_on_late` and
`a_unit_past_the_ring` pin down what happens instead.
"""
import functools

import numpy as np

import viz_player_cases as K
from framer_features_oracle import make_events, DELTA_T, ABSOLUTE_T

W = H = 9
CFG = K.base_cfg(W, H, 1, buffer_limit=1)
CFG_ABS = K.base_cfg(W, H, 1, buffer_limit=1, time_mode=ABSOLUTE_T)
CFG_RGB = K.base_cfg(W, H, 3, buffer_limit=1)

FULL = [(x, y, None, 7, 255) for y in range(H) for x in range(W)]
FULL_RGB = [(x, y, c, 7, 255) for y in range(H) for x in range(W) for c in range(3)]
DUMMY = (8, 0, None, 7, 100)  # a border event that only provides a last_event
CENTRE = (4, 4, None, 0, 200)
ALL_ROWS = range(H)


def jumps(rows=ALL_ROWS, t=765, c=None):
    return [(0, y, c, 7, t) for y in rows]


def frame(base, cells=(), channels=1):
    """[H][W][channels] u8: `base` everywhere, then cells = {(x, y) or (x, y, c): value}"""
    f = np.full((H, W, channels), base, np.uint8)
    for key, v in dict(cells).items():
        if len(key) == 2:
            f[key[1], key[0], :] = v
        else:
            f[key[1], key[0], key[2]] = v
    return f


def cross(x, y):
    """adder.rs:359-388: radius 2, both arms"""
    return {**{(x, y + i): 255 for i in range(-2, 3)}, **{(x + i, y): 255 for i in range(-2, 3)}}


def col0(v, rows=ALL_ROWS):
    return {(0, y): v for y in rows}


def call(features=(), pops=(), intervals=(), popped=None, running=None, plane=None, error=False):
    """error: frame_features reports a feature that could not be filed (the reference would have panicked)"""
    return dict(features=[tuple(f) for f in features], pops=list(pops),
                intervals=[(e, [tuple(p) for p in xy]) for e, xy in intervals], popped=popped, running=running,
                plane=plane, error=error)


def case(name, cfg, ops, calls, ring_frames=1024):
    return dict(name=name, cfg=cfg, ops=ops, calls=calls, ring_frames=ring_frames)


NOT_3 = [y for y in ALL_ROWS if y != 3]
F0 = frame(128)
# the frames of `cascade_and_crosses` (see there)
_C1P = frame(0, {(8, 0): 255, (4, 4): 1, (3, 3): 0, **col0(42, NOT_3)})
_C1R = frame(128, {(8, 0): 255, (3, 3): 0, **col0(42, NOT_3), **cross(4, 4)})
_C2P = frame(0, col0(42, NOT_3))
_C2R = frame(128, {(8, 0): 255, **col0(42, NOT_3), **cross(4, 4), **cross(3, 3)})
_C3 = frame(128, {(4, 4): 64, (3, 3): 0, (8, 0): 32, **col0(42, NOT_3)})
_C4P = frame(0, {(8, 0): 32})
_CASCADE_CALLS = [
    # events 0..80 FULL, 81 DUMMY, 82 CENTRE (1 under a ring of 128: a corner; t 200: idx 0 -> the interval ending 510),
    # 83 (3, 3) -> 0 under 128s: a corner; t 600, frames_written 1: idx 600 / 255 - 1 = 1 -> the deque [510] grows by 765.
    # (3, 3) reaches frame 3 and forces row 3; the jumps 84..91 force the other rows: frame 1 pops at P = 91 with the
    # interval (510, [(4, 4)]), frame 2 right after it with (765, [(3, 3)]).
    # Frame 1: Some are (8, 0) 255, (4, 4) 1, (3, 3) 0 and the jumped (0, y) 42; the cross of (4, 4) then wins over its 1.
    # Frame 2: Some are (3, 3) 0 and the (0, y); (4, 4)'s cross pixels are None there and stay; the cross of (3, 3)
    # wins over its 0.
    call(features=[(82, 200, 4, 4), (83, 600, 3, 3)], pops=[80, 91, 91],
         intervals=[(255, []), (510, [(4, 4)]), (765, [(3, 3)])], popped=[F0, _C1P, _C2P], running=[F0, _C1R, _C2R]),
    # 92: (4, 4) + 510 -> clock 1020, frames 2..3 (2 is late), value 64; the first event of a period.  93: (8, 0) runs to
    # frame 5 (value 32) and forces row 0 only: nothing pops.
    call(),
    # finish: frame 3 is flushed (every None takes its unit's last intensity) and pops with (1020, []); every cross
    # pixel is Some there and is overwritten.  Then 5 - 4 + 1 > 1: frame 4 pops unflushed, only (8, 0) is Some.
    call(pops=[93, 93], intervals=[(1020, []), (1275, [])], popped=[_C3, _C4P], running=[_C3, _C3],
         plane=frame(128, {(4, 4): 64, (3, 3): 0, (8, 0): 32, **col0(42, NOT_3)})),
]
_CASCADE_EVENTS = FULL + [DUMMY, CENTRE, (3, 3, None, 0, 600)] + jumps(NOT_3)
_TAIL = [(4, 4, None, 7, 510), (8, 0, None, 7, 1000)]

# tps 3 932 160 at 30 fps: tpf = 2^17 = 131 072 (ref_interval stays 255: (d 7, t 255) -> 128)
CFG_WIDE = K.base_cfg(W, H, 1, buffer_limit=None, tps=3932160)
TPF_WIDE = 131072
FULL_2 = [(x, y, None, 15, 200000) for y in range(H) for x in range(W)]  # every unit into frame 1: 2^15 / 200000 * 255 -> 41
_WIDE_1 = frame(41, {(4, 4): 0})

CASES = [
    # event 81 is the first one `consume` reads after the pop at P = 80: last_event is None
    case("the_first_event_of_a_period_is_not_tested", CFG,
         [("detect", True), ("ingest", FULL + [CENTRE])],
         [call(pops=[80], intervals=[(255, [])], popped=[F0], running=[F0], plane=frame(128, {(4, 4): 1}))]),
    # the same centre event one later: last.t = 100 != 200, the ring is 128 > 1 + 30 all round
    case("the_same_event_in_mid_period_is_a_feature", CFG,
         [("detect", True), ("ingest", FULL + [DUMMY, CENTRE]), ("finish",)],
         [call(features=[(82, 200, 4, 4)], pops=[80], intervals=[(255, [])], popped=[F0], running=[F0]),
          call()]),  # the largest last_filled is 1 = frames_written: nothing to flush
    # 81..89 force every row: frames 1 and 2 pop at P = 89, frames_written 3.  90: (0, 0) -> frame 4.  91 CENTRE reaches
    # frame 1 only: late, dropped -- and still writes 1 into the plane and is a corner.  t 200 -> idx 0: the interval
    # ending 1020, which the flushed frame 3 takes at finish, with its cross.
    case("a_late_dropped_event_is_a_feature_and_finish_takes_its_interval", CFG,
         [("detect", True), ("ingest", FULL + jumps() + [(0, 0, None, 7, 100), CENTRE]), ("finish",)],
         [call(features=[(91, 200, 4, 4)], pops=[80, 89, 89], intervals=[(255, []), (510, []), (765, [])],
               popped=[F0, frame(0, col0(42)), frame(0, col0(42))],
               running=[F0, frame(128, col0(42)), frame(128, col0(42))]),
          call(pops=[91], intervals=[(1020, [(4, 4)])], popped=[frame(128, {**col0(42), (4, 4): 1})],
               running=[frame(128, {**col0(42), **cross(4, 4)})],
               plane=frame(128, {**col0(42), (0, 0): 255, (4, 4): 1}))]),
    # AbsoluteT, the same feature time 700 in two periods.  frames_written 1: idx = 700 / 255 - 1 = 1, the interval ending
    # 765.  (The jumps at t 1275 reach frame 4: frames 1..3 pop and show where it went.)
    case("absolute_t_feature_is_filed_under_its_periods_frames_written", CFG_ABS,
         [("detect", True), ("ingest", FULL + [(1, 0, None, 7, 300), (4, 4, None, 0, 700)] + jumps(t=1275))],
         [call(features=[(82, 700, 4, 4)], pops=[80, 91, 91, 91],
               intervals=[(255, []), (510, []), (765, [(4, 4)]), (1020, [])])]),
    # ... after a forced pop (jumps at 1020: frames 1, 2 pop at P = 89) frames_written is 3 > 700 / 255: idx 0, the
    # interval ending 1020 -- one index earlier.  (1, 0) at 90 opens the period; the jumps at 1785 reach frame 6.
    case("absolute_t_feature_after_a_forced_pop_is_filed_one_index_earlier", CFG_ABS,
         [("detect", True),
          ("ingest", FULL + jumps(t=1020) + [(1, 0, None, 7, 300), (4, 4, None, 0, 700)] + jumps(t=1785))],
         [call(features=[(91, 700, 4, 4)], pops=[80, 89, 89, 100, 100, 100],
               intervals=[(255, []), (510, []), (765, []), (1020, [(4, 4)]), (1275, []), (1530, [])])]),
    case("cascade_and_crosses", CFG,
         [("detect", True), ("ingest", _CASCADE_EVENTS), ("ingest", _TAIL), ("finish",)], _CASCADE_CALLS),
    # three channels, ring and centre on channel 0; the cross takes all three bytes of its nine pixels
    case("three_channels_get_three_bytes", CFG_RGB,
         [("detect", True), ("ingest", FULL_RGB + [(8, 0, 0, 7, 100), (4, 4, 0, 0, 200)] + jumps(c=0))],
         [call(features=[(244, 200, 4, 4)], pops=[242, 253, 253], intervals=[(255, []), (510, [(4, 4)]), (765, [])],
               popped=[frame(128, channels=3),
                       frame(0, {(8, 0, 0): 255, (4, 4, 0): 1, **{(0, y, 0): 42 for y in ALL_ROWS}}, 3),
                       frame(0, {(0, y, 0): 42 for y in ALL_ROWS}, 3)],
               running=[frame(128, channels=3)] +
               [frame(128, {(8, 0, 0): 255, **{(0, y, 0): 42 for y in ALL_ROWS}, **cross(4, 4)}, 3)] * 2)]),
    # FULL with detection off: the plane stays 0 and frame 0's pop takes (255, []) all the same.  Then (4, 4) -> 128 over
    # zeros is a corner; t 255, frames_written 1: idx 0, the interval the running deque has there ends at 510 >= 255:
    # nothing is raised (the framer's case of the same name raises, its deque did not run)
    case("detection_switched_on_late", CFG,
         [("ingest", FULL), ("detect", True), ("ingest", [DUMMY, (4, 4, None, 7, 255)] + jumps())],
         [call(pops=[80], intervals=[(255, [])], popped=[F0], running=[F0], plane=frame(0)),
          call(features=[(82, 255, 4, 4)], pops=[91, 91], intervals=[(510, [(4, 4)]), (765, [])],
               plane=frame(0, {(8, 0): 255, (4, 4): 128, **col0(42)}))]),
    # `cascade_and_crosses` again, with calls in between that are refused (they change nothing: plane, carried event,
    # deque, crosses) and a bad event at index 8 (commits as if the batch had ended before it)
    case("refused_calls_change_nothing", CFG,
         [("detect", True), ("ingest", _CASCADE_EVENTS[:84]),
          ("refused_capacity", _CASCADE_EVENTS[84:], 2),
          ("refused_ring", [(4, 4, None, 0, 255 * 5000)]),
          ("bad_event", _CASCADE_EVENTS[84:] + [(9, 0, None, 7, 5), CENTRE], 8),
          ("refused_ring", [CENTRE, (4, 4, None, 0, 255 * 5000)]),
          ("ingest", _TAIL), ("finish",)],
         [call(features=[(82, 200, 4, 4), (83, 600, 3, 3)], pops=[80], intervals=[(255, [])], popped=[F0], running=[F0]),
          call(pops=[91, 91], intervals=[(510, [(4, 4)]), (765, [(3, 3)])], popped=[_C1P, _C2P], running=[_C1R, _C2R]),
          _CASCADE_CALLS[1], _CASCADE_CALLS[2]]),
    # DeltaT, no limit, a ring of 65536 frames.  FULL: frame 0 pops at P = 80 with (131072, []), the deque is [262144].
    # 81 (8, 0) + 300 stays in frame 0.  82: (4, 4) + 0xFFFFFFFF -> clock 4 294 967 550, frames 1..32768 (inside the
    # ring), value 1 / 0xFFFFFFFF * 255 -> 0 under a ring of 128s: a corner, listed.  time / tpf = 32767 >= 1: idx 32766;
    # the new end (32767 + 1) * 2^17 wraps to 0, nothing grows, idx >= 1 = the deque's length: the reference panics, the
    # feature is not filed and frame_features says so from here on.
    # FULL_2 (83..163) puts every unit into frame 1 (equal t: none is tested); it is complete at P = 163 and pops with
    # (262144, []): (4, 4) holds the 0 of event 82 there, the others 41.  Frames and pops go on.
    # 164 (8, 0) opens a period; 165: (3, 3) + 131072 -> frame 2, value 0 under 41s: a corner, listed, not filed.
    # reset: the state of a fresh context.  (4, 4) + 131072 -> frame 1, 0 under 128s: a corner at t 131072, idx 1 - 1 = 0:
    # the interval ending 262144, popped with frame 1 and its cross; nothing is reported any more.
    case("a_feature_past_the_deque_is_reported_while_frames_go_on", CFG_WIDE,
         [("detect", True), ("ingest", FULL + [(8, 0, None, 7, 300), (4, 4, None, 0, 0xFFFFFFFF)]), ("ingest", FULL_2),
          ("ingest", [(8, 0, None, 7, 100), (3, 3, None, 0, TPF_WIDE)]),
          ("reset",), ("ingest", FULL + [(8, 0, None, 7, 300), (4, 4, None, 0, TPF_WIDE)] + FULL_2)],
         [call(features=[(82, 0xFFFFFFFF, 4, 4)], pops=[80], intervals=[(TPF_WIDE, [])], popped=[F0], running=[F0],
               plane=frame(128, {(4, 4): 0}), error=True),
          call(pops=[163], intervals=[(2 * TPF_WIDE, [])], popped=[_WIDE_1], running=[_WIDE_1], plane=frame(41), error=True),
          call(features=[(165, TPF_WIDE, 3, 3)], plane=frame(41, {(3, 3): 0}), error=True),
          call(features=[(82, TPF_WIDE, 4, 4)], pops=[80, 163], intervals=[(TPF_WIDE, []), (2 * TPF_WIDE, [(4, 4)])],
               popped=[F0, _WIDE_1], running=[F0, frame(41, cross(4, 4))], plane=frame(41))],
         ring_frames=65536),
    # a t that would wrap (time / tpf + 1) * tpf in u32 sends its unit 16 843 009 frames ahead: refused, nothing changes
    case("a_unit_past_the_ring", CFG,
         [("detect", True), ("ingest", FULL + [DUMMY]), ("refused_ring", [(4, 4, None, 0, 0xFFFFFFFF)]),
          ("ingest", [CENTRE])],
         [call(pops=[80], intervals=[(255, [])]), call(features=[(82, 200, 4, 4)], plane=frame(128, {(8, 0): 255, (4, 4): 1}))]),
]


def run(impl, ops):
    """impl: detect_features(on), set_buffer_limit(l), ingest(events) / finish() -> dict(features, pops, intervals,
    popped, running), plane(), refused(kind, events, arg) (asserts the refusal; a no-op for a restatement),
    bad_event(events, b) -> as ingest.  -> the log of every ingest / bad_event / finish call"""
    log = []
    for op in ops:
        if op[0] == "detect":
            impl.detect_features(op[1])
        elif op[0] == "limit":
            impl.set_buffer_limit(op[1])
        elif op[0] == "ingest":
            log.append(impl.ingest(make_events(op[1])))
        elif op[0] == "bad_event":
            log.append(impl.bad_event(make_events(op[1]), op[2]))
        elif op[0] == "finish":
            log.append(impl.finish())
        elif op[0] == "reset":
            impl.reset()
        elif op[0] in ("refused_capacity", "refused_ring"):
            impl.refused(op[0], make_events(op[1]), op[2] if len(op) > 2 else None)
        if op[0] in ("ingest", "bad_event", "finish"):
            log[-1]["plane"] = impl.plane()
    return log


def check(case_, log):
    """the log of `run` against the case's known answers"""
    name = case_["name"]
    assert len(log) == len(case_["calls"]), name
    for k, (got, want) in enumerate(zip(log, case_["calls"])):
        at = (name, k)
        assert [tuple(f) for f in got["features"]] == want["features"], at
        assert list(got["pops"]) == want["pops"], at
        assert got["intervals"] == want["intervals"], at
        assert got["error"] == want["error"], at
        for form in ("popped", "running"):
            if want[form] is not None:
                assert len(got[form]) == len(want[form]), at + (form,)
                for j, f in enumerate(want[form]):
                    assert np.array_equal(np.asarray(got[form][j]).reshape(f.shape), f), at + (form, j)
        if want["plane"] is not None:
            assert np.array_equal(np.asarray(got["plane"]).reshape(want["plane"].shape), want["plane"]), at + ("plane",)


class RestatementImpl:
    """tests/viz_features_oracle.py behind the interface of `run`"""

    def __init__(self, cfg):
        from viz_features_oracle import VizFeatureRestatement
        self.cfg = cfg
        self.r = VizFeatureRestatement(**cfg)

    def reset(self):
        """the state of a fresh context; detection and the limit as they stand"""
        from viz_features_oracle import VizFeatureRestatement
        old = self.r
        self.r = VizFeatureRestatement(**dict(self.cfg, buffer_limit=old.buffer_limit))
        self.r.detect_features(old.detect)

    def detect_features(self, on):
        self.r.detect_features(on)

    def set_buffer_limit(self, limit):
        self.r.set_buffer_limit(limit)

    def _log(self, popped, features):
        return dict(features=[(int(f["index"]), int(f["t"]), int(f["x"]), int(f["y"])) for f in features],
                    pops=[int(p[0]) for p in popped], intervals=list(self.r.last_intervals),
                    error=self.r.broken is not None,
                    popped=[p[1] for p in popped], running=[p[3] for p in popped])

    def ingest(self, events):
        return self._log(self.r.feed(events), self.r.last_features)

    def bad_event(self, events, b):
        return self.ingest(events[:b])

    def finish(self):
        return self._log(self.r.finish(), [])

    def refused(self, kind, events, arg):
        pass

    def plane(self):
        return self.r.running_intensities.copy()

    def running_frame(self):
        return self.r.running.copy()


# ---- seeded streams: the smallest planes at which the kernels can go wrong -----------------------------------------

SEEDED = {  # width, height, channels, events
    "9x8": (9, 8, 1, 3000),
    "12x9rgb": (12, 9, 3, 4000),
    "70x9": (70, 9, 1, 4000),  # a row past a wave
    "300x8": (300, 8, 1, 10000),  # a row past a 256-thread block
}
LIMITS = (1, 2, 60, None)


def seeded_stream(name, time_mode):
    """gen_sweep (a camera-like stream; d 0..8 spreads the intensities over 1..255, so corners abound) with a
    gen_stream tail (bursts, lagging rows); AbsoluteT streams hold events from their unit's past"""
    w, h, c, n = SEEDED[name]
    past = 0.1 if time_mode == ABSOLUTE_T else 0.0
    if time_mode == ABSOLUTE_T:
        return K.gen_sweep(7, w, h, c, n, time_mode=time_mode, past=past, slow_rows=0.3)
    head = K.gen_sweep(7, w, h, c, n - n // 4, time_mode=time_mode, past=past, slow_rows=0.3)
    return np.concatenate([head, K.gen_stream(8, w, h, c, n // 4, max_step=2)])


def seeded_cfg(name, time_mode, limit):
    w, h, c, _ = SEEDED[name]
    return K.base_cfg(w, h, c, time_mode=time_mode, buffer_limit=limit)


@functools.lru_cache(maxsize=None)
def seeded(name, time_mode, limit):
    """-> (cfg, events, the restatement after feed (one call, detection on) + finish, frames before the drain, the
    features of the feed); computed once, shared by the tests, left unchanged"""
    from viz_features_oracle import VizFeatureRestatement
    cfg = seeded_cfg(name, time_mode, limit)
    ev = seeded_stream(name, time_mode)
    r = VizFeatureRestatement(**cfg)
    r.detect_features(True)
    r.feed(ev)
    feats = r.last_features
    before = len(r.popped)
    r.finish()
    return cfg, ev, r, before, feats
