"""Literal pure-Python restatement of the reference's adder_video_player (adder-codec-rs/src/bin_cv/
adder_video_player.rs:52-216, framer/scale_intensity.rs:262-270) -- the yardstick of the latest-event player
(include/adder_player.h).  Times are Python ints masked to 32 bits (the release build's wrapping u32), values are
Python floats (binary64).  One loop iteration per record, with the display check first.

Errors follow the library's definition: an event with d <= 128 outside the plane stops the run as if the batch had
ended before it.

numpy_restate() is the same computation vectorised, for planes too large for the loop; it is held against the loop
in tests/test_player_cpu.py.
"""
import numpy as np

D_ZERO_INTEGRATION = 128
ABSOLUTE_T = 1
MASK = 0xFFFFFFFF
MAX_INTENSITY = {0: 255.0, 1: 65535.0, 2: 4294967295.0, 3: float((1 << 64) - 1), 6: 255.0, 7: 255.0}


def frame_length(tps, playback_fps):
    """(tps as f64 / playback_fps) as u128: truncated, saturating"""
    q = float(tps) / playback_fps
    return (1 << 128) - 1 if q >= 2.0 ** 128 else int(q)


def event_to_intensity(d, t):
    if d > D_ZERO_INTEGRATION:
        return 0.0
    p = 0.0 if d == D_ZERO_INTEGRATION else float(1 << d)
    return p if t == 0 else p / float(t)


def round_up(ts, ref):
    return ts if ts % ref == 0 else ((ts // ref + 1) * ref) & MASK


def serial_schedule(cur_before, f0, fl):
    """The display checks on their own: cur_before[i] = current_t at check i -> (marks, frame_count after)."""
    marks, f = [], f0
    for cur in cur_before:
        show = int(cur) > f * fl
        marks.append(1 if show else 0)
        f += 1 if show else 0
    return marks, f


class PlayerRestatement:
    def __init__(self, width, height, channels, time_mode, ref_interval, tps, source_camera, playback_fps=60.0):
        self.w, self.h, self.ch = width, height, channels
        self.absolute = time_mode == ABSOLUTE_T
        self.ref = ref_interval
        self.m = MAX_INTENSITY[source_camera]  # KeyError: todo!() in the reference
        self.fl = frame_length(tps, playback_fps)
        self.last_ts = np.zeros((height, width, channels), np.uint32)
        self.display = np.zeros((height, width, channels), np.float64)
        self.current_t = 0
        self.frame_count = 1

    @classmethod
    def from_meta(cls, meta, playback_fps=60.0):
        return cls(meta["width"], meta["height"], meta["channels"], meta["time_mode"], meta["ref_interval"],
                   meta["tps"], meta["source_camera"], playback_fps)

    def check(self, frames):
        if self.current_t > self.frame_count * self.fl:
            frames.append(self.display.copy())
            self.frame_count += 1

    def run(self, events, end=False):
        """events: an EVENT_DTYPE array or an iterable of (x, y, c, d, t) (c 0xFF = None).  end: the stream ends behind
        them (the iteration that meets the EOF makes one more check).  -> (frames, bad index or None)"""
        frames = []
        if hasattr(events, "dtype"):
            events = zip(events["x"].tolist(), events["y"].tolist(), events["c"].tolist(), events["d"].tolist(),
                         events["t"].tolist())
        ref = self.ref
        for k, (x, y, c, d, t) in enumerate(events):
            c = 0 if c == 0xFF else c
            if d <= D_ZERO_INTEGRATION and not (x < self.w and y < self.h and c < self.ch):
                return frames, k  # ours: as if the batch had ended before k (no check at k)
            self.check(frames)
            if d > D_ZERO_INTEGRATION:
                continue
            last = int(self.last_ts[y, x, c])
            if self.absolute:
                if t > self.current_t:
                    self.current_t = t
                dt = (t - last) & MASK
                self.last_ts[y, x, c] = round_up(t, ref)
                t = dt
            else:
                last = round_up((last + t) & MASK, ref)
                self.last_ts[y, x, c] = last
                if last > self.current_t:
                    self.current_t = last
            self.display[y, x, c] = (event_to_intensity(d, t) * float(ref)) / self.m
        if end:
            self.check(frames)
        return frames, None

    def finish(self):
        frames = []
        self.check(frames)
        return frames


def to_u8(frame):
    """ADDER_PLAYER_U8: saturate(rint(v * 255)), ties to even"""
    return np.clip(np.rint(frame * 255.0), 0, 255).astype(np.uint8)


def numpy_restate(meta, ev, playback_fps=60.0, end=True):
    """The same run from a fresh state in vectorised numpy (in-plane events only): -> (frames, final matrix, current_t,
    frame_count).  The per-unit chains are cumulative sums per unit, which is exact while no time wraps (asserted)."""
    w, h, ch, ref = meta["width"], meta["height"], meta["channels"], meta["ref_interval"]
    absolute = meta["time_mode"] == ABSOLUTE_T
    m = MAX_INTENSITY[meta["source_camera"]]
    fl = frame_length(meta["tps"], playback_fps)
    n = len(ev)
    c = np.where(ev["c"] == 0xFF, 0, ev["c"]).astype(np.int64)
    unit = (ev["y"].astype(np.int64) * w + ev["x"]) * ch + c
    valid = ev["d"] <= D_ZERO_INTEGRATION
    order = np.flatnonzero(valid)[np.argsort(unit[valid], kind="stable")]
    u_s, t_s, d_s = unit[order], ev["t"][order].astype(np.int64), ev["d"][order].astype(np.int64)
    head = np.ones(len(order), bool)
    head[1:] = u_s[1:] != u_s[:-1]
    rnd = lambda a: np.where(a % ref == 0, a, (a // ref + 1) * ref)
    if absolute:
        prev = np.where(head, 0, np.roll(rnd(t_s), 1))
        tt = (t_s - prev) & MASK
        cand_s = t_s
    else:
        # last_ts after each event of a run: every term is rounded, so walk the runs in lock step by rank
        ts = np.zeros(len(order), np.int64)
        start = np.flatnonzero(head)
        length = np.diff(np.append(start, len(order)))
        acc = np.zeros(len(start), np.int64)
        for r in range(int(length.max()) if len(length) else 0):
            live = length > r
            acc[live] = rnd(acc[live] + t_s[start[live] + r])
            ts[start[live] + r] = acc[live]
        assert ts.max(initial=0) <= MASK
        tt = t_s
        cand_s = ts
    p = np.where(d_s == 128, 0.0, np.ldexp(1.0, np.minimum(d_s, 127).astype(np.int32)))
    inten = np.where(tt == 0, p, p / np.maximum(tt, 1).astype(np.float64))
    val_s = (inten * float(ref)) / m
    cand = np.zeros(n + 1, np.int64)
    cand[order + 1] = cand_s
    cur_before = np.maximum.accumulate(cand)  # cur_before[i]: after the events before i
    nchk = n + 1 if end else n
    marks, fc = serial_schedule(cur_before[:nchk].tolist(), 1, fl)
    frames = []
    for s in np.flatnonzero(np.array(marks, bool)):
        f = np.zeros(w * h * ch)
        sel = order < s  # per unit the last such event wins: order is stable, so later assignments are later events
        f[u_s[sel]] = val_s[sel]
        frames.append(f.reshape(h, w, ch))
    final = np.zeros(w * h * ch)
    final[u_s] = val_s
    return frames, final.reshape(h, w, ch), int(cur_before[n]), fc
