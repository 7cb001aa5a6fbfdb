"""Python restatement of the adder-viz player with feature detection (adder-viz/src/player/adder.rs:281-282, 319-440)
-- test helper.

A subclass of VizRestatement (tests/viz_player_oracle.py: `consume` over the buffer-limited FrameSequence) that adds,
literally: the detect_features block of Framer::ingest_event (driver.rs:482-553), pop_features (:851-873) after every
popped frame, `last_event = None` each time `consume` is entered (adder.rs:409), `last_event = Some(event)` with the t
ingest_event_for_chunk left in it (driver.rs:1022-1028), and the cross painting of adder.rs:359-388.  The corner test
(`_is_feature`), the plane and the FeatureInterval deque with `_file` are framer_features_oracle.Restatement's, used
through one instance of it.  Nothing here knows of periods, W_i, stamps or cursors: those are the product's
decomposition (include/adder_viz_player.h), which the tests hold against this.

Around the reference's functions it adds what the header defines: last_event carried from feed() to feed() (a call
boundary is not a `consume` boundary), cleared by detect_features() and set_buffer_limit(); the features of the last
feed() with their global stream index; one interval per popped frame in `intervals`, aligned with `popped`.  Where the
reference would panic (Restatement.broken), later features are not filed and the pops go on.

`per_consume_reset=False` is for tests only: it leaves last_event alone when `consume` is entered, which makes the
features those of the framer's restatement.
"""
import numpy as np

from framer_features_oracle import Restatement, FEATURE_DTYPE, D_EMPTY, U32
from viz_player_oracle import VizRestatement, VIEW_SAE


class VizFeatureRestatement(VizRestatement):
    def __init__(self, width, height, channels=1, *, per_consume_reset=True, **kw):
        super().__init__(width, height, channels, **kw)
        fkw = {k: kw[k] for k in ("tps", "ref_interval", "delta_t_max") if k in kw}
        self.F = Restatement(width, height, channels, output_fps=kw.get("output_fps"), **fkw)
        assert self.F.tpf == self.tpf
        self.detect = False
        self.per_consume_reset = per_consume_reset
        self.last = None          # last_event.t of the running `consume` (None: no last event)
        self.intervals = []       # per popped frame: (end_ts, [(x, y)])
        self.last_features = np.zeros(0, FEATURE_DTYPE)
        self.last_intervals = []
        self._feats = []
        self._in_finish = False
        # census (no part of the restated logic)
        self._prev_t = None       # the t left in the previous event, whatever `consume` it belonged to
        self._cross = np.zeros(height * self.px, bool)  # units that show a cross
        self.c_late_features = 0      # features of events that were dropped as late for a frame
        self.c_suppressed = 0         # corners not tested only because their event opened a `consume`
        self.c_cross_kept = 0         # (unit, frame): a cross kept across a None
        self.c_cross_overwritten = 0  # (unit, frame): a cross overwritten by a Some
        self.c_iv_forced = 0          # intervals with features popped by the first pop of a forced return
        self.c_iv_cascade = 0         # ... by a later pop of one loop
        self.c_iv_finish = 0          # ... by a pop of the Err arm
        self.c_idx_above_0 = 0        # features filed at an index above 0

    # ---- the plane and the deque live in the framer's restatement ----
    @property
    def running_intensities(self):
        return self.F.running

    @property
    def broken(self):
        return self.F.broken

    def detect_features(self, on):
        self.detect = bool(on)
        self.last = None  # a UI update lies between two `consume` calls

    def set_buffer_limit(self, buffer_limit):
        super().set_buffer_limit(buffer_limit)
        self.last = None

    # ---- Framer::ingest_event (driver.rs:437-562) ----
    def ingest_event(self, x, y, c, d, t):
        cc = 0 if c == 0xFF else c
        off = x * self.ch + cc
        time = t
        # the t ingest_event_for_chunk leaves in the event (driver.rs:1002-1028)
        prev_ts, prev_lastf = self.ts[y][off], self.lastf[y][off]
        t_after = t
        if self.abs_t and prev_ts < t:
            if max(t - 1, 0) // self.tpf > prev_lastf and d != D_EMPTY and self.view != VIEW_SAE:
                t_after = max(t - (prev_ts & U32), 0)
        late_before = self.late_drops
        filled = super().ingest_event(x, y, c, d, t)
        if self.detect:
            self.F.running[y, x, cc] = min(self.lasti[y][off], 255)
            differs = lambda last: last is not None and time != last
            if differs(self.last):
                if self.F._is_feature(x, y, c):
                    self._feats.append((self.n_ingested - 1, time, x, y))
                    self.F.frames_written = self.frames_written
                    if not self.F.broken:
                        idx = ((time // self.tpf) - (self.frames_written & U32)) & U32 \
                            if time // self.tpf >= self.frames_written else 0
                        if time % self.tpf == 0 and idx > 0:
                            idx -= 1
                        self.c_idx_above_0 += idx > 0
                    self.F._file(time, x, y)
                    self.c_late_features += self.late_drops > late_before
            elif differs(self._prev_t) and self.F._is_feature(x, y, c):
                self.c_suppressed += 1
        self.last = self._prev_t = t_after  # last_event = Some(event) (adder.rs:417)
        return filled

    # ---- FrameSequence::pop_features (driver.rs:851-873); a deque the reference would have panicked over goes on ----
    def _pop_features(self):
        dq = self.F.features
        if not dq:
            dq.append([self.tpf, []])
            dq.append([self.tpf * 2, []])
        else:
            dq.append([self.tpf + dq[-1][0], []])
        return dq.popleft()

    # ---- adder.rs:339-409: the loop in front of the read loop, then last_event = None ----
    def _show(self, returned=False):
        forced = any(self.row_forced)
        if returned:
            if forced:
                self.forced_pops += 1
            else:
                self.natural_pops += 1
        first = len(self.popped)
        width, color_channels = self.w, self.ch
        is_color = color_channels == 3
        while self.is_frame_0_filled():
            new_frame = self.pop_next_frame()
            val = np.concatenate([f.val for f in new_frame])
            some = np.concatenate([f.some for f in new_frame])
            db = self.running
            db[some] = val[some]
            self.c_cross_kept += int((self._cross & ~some).sum())
            self.c_cross_overwritten += int((self._cross & some).sum())
            self._cross &= ~some
            end_ts, features = self._pop_features()
            for fx, fy in features:
                color, radius = 255, 2
                for i in range(-radius, radius + 1):
                    idx = (fy + i) * width * color_channels + fx * color_channels
                    db[idx] = color
                    self._cross[idx] = True
                    if is_color:
                        db[idx + 1] = db[idx + 2] = color
                        self._cross[idx + 1] = self._cross[idx + 2] = True
                    idx = fy * width * color_channels + (fx + i) * color_channels
                    db[idx] = color
                    self._cross[idx] = True
                    if is_color:
                        db[idx + 1] = db[idx + 2] = color
                        self._cross[idx + 1] = self._cross[idx + 2] = True
            if features:
                k = len(self.popped) - first
                if self._in_finish:
                    self.c_iv_finish += 1
                elif k > 0:
                    self.c_iv_cascade += 1
                elif returned and forced:
                    self.c_iv_forced += 1
            self.popped.append((self.n_ingested - 1, np.where(some, val, 0).astype(np.uint8), some, db.copy()))
            self.intervals.append((end_ts, [(int(a), int(b)) for a, b in features]))
        self.longest_cascade = max(self.longest_cascade, len(self.popped) - first)
        if self.per_consume_reset:
            self.last = None  # `let mut last_event: Option<Event> = None` (adder.rs:409)

    def feed(self, events):
        self._feats = []
        n0 = len(self.intervals)
        out = super().feed(events)
        self.last_features = np.array(self._feats, FEATURE_DTYPE) if self._feats else np.zeros(0, FEATURE_DTYPE)
        self.last_intervals = self.intervals[n0:]
        return out

    def finish(self):
        n0 = len(self.intervals)
        self._in_finish = True
        out = super().finish()
        self._in_finish = False
        self.last_intervals = self.intervals[n0:]
        return out
