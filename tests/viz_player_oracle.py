"""Python restatement of the adder-viz player (adder-viz/src/player/adder.rs:319-440, `consume`) over the framer it
drives (adder-codec-rs/src/framer/driver.rs: ingest_event :437-562, flush_frame_buffer :632-677, is_frame_0_filled
:828-843, pop_next_frame :878-925, ingest_event_for_chunk :984-1133) -- test helper.

Literal: one deque of Option<u8> frames per chunk (chunk_rows = 1, so per row), filled_count per frame, the
chunk_filled_tracker, frame_idx_offsets, the `while is_frame_0_filled()` loop in front of the read loop, the return at
the first event whose ingest_event is true, and the Err arm where flush_frame_buffer and the consume recursion
alternate.  It keeps the Option masks and the running frame.  Nothing here knows of periods, coverage counts or pop
schedules: those are the product's decomposition (include/adder_viz_player.h), which the tests hold against this.

`VizRestatement.feed(events)` is `consume` called again and again over one shared stream position until the events run
out WITHOUT meeting the end of the stream (the product's ingest); `finish()` is the Err arm.  Each popped frame is
recorded as (P, values, some, running): P = the global index of the last event ingested before the pop (-1: none).
"""
import collections

import numpy as np

from framer_features_oracle import get_frame_value, _as_uint, f32, EVENT_DTYPE, D_EMPTY, U32  # noqa: F401

DELTA_T, ABSOLUTE_T = 0, 1
VIEW_SAE = 3


class _Frame:
    __slots__ = ("val", "some", "filled_count")

    def __init__(self, px):
        self.val = np.zeros(px, np.uint8)
        self.some = np.zeros(px, bool)
        self.filled_count = 0


class VizRestatement:
    def __init__(self, width, height, channels=1, *, tps, ref_interval, delta_t_max, output_fps, codec_version=2,
                 time_mode=DELTA_T, source_camera=0, buffer_limit=60, view_mode=0, source_type=0, practical_d_max=0.0):
        self.w, self.h, self.ch = width, height, channels
        self.px = width * channels  # array.len() of one chunk: FramerBuilder::new(plane, 1)
        self.ref_interval, self.delta_t_max = ref_interval, delta_t_max
        self.tpf = ref_interval if output_fps is None else _as_uint(f32(tps) / f32(output_fps), 4294967295.0)
        self.abs_t = codec_version >= 2 and time_mode == ABSOLUTE_T
        self.round_up = codec_version >= 1 and source_camera <= 5
        self.view, self.source, self.pdm = view_mode, source_type, practical_d_max
        self.buffer_limit = buffer_limit  # Option<u32>
        self.frames_written = 0
        self.frames = [collections.deque([_Frame(self.px)]) for _ in range(height)]
        self.frame_idx_offsets = [0] * height
        self.chunk_filled = [False] * height
        self.ts = [[0] * self.px for _ in range(height)]
        self.lastf = [[-1] * self.px for _ in range(height)]
        self.lasti = [[0] * self.px for _ in range(height)]
        self.running = np.zeros(height * self.px, np.uint8)
        self.limit_set = False
        self.n_ingested = 0   # events handed to ingest_event since creation
        self.popped = []      # (P, values u8 [h*w*c], some bool, running u8 copy)
        # census (what the streams of a test reach; no part of the restated logic)
        self.late_drops = 0       # fills of frames already popped
        self.flushes = 0          # frames flush_frame_buffer completed
        self.row_forced = [False] * height
        self.forced_pops = 0      # `consume` returns where some row's frame 0 was forced
        self.natural_pops = 0     # ... where no row's was
        self.stalls = 0           # a row is forced while another row keeps ingest_event false
        self.longest_cascade = 0  # frames shown by one run of the loop in front of the read loop
        self.past_events = 0      # AbsoluteT events from their unit's past
        self.past_would_force = 0  # ... whose unit is more than buffer_limit frames ahead

    # ---- ingest_event_for_chunk (driver.rs:984-1133), off = the unit inside its row ----
    def _chunk(self, r, off, d, t):
        chunk = self.frames[r]
        prev_lastf, prev_ts = self.lastf[r][off], self.ts[r][off]
        if self.abs_t:
            if prev_ts >= t:
                self.past_events += 1
                if self.buffer_limit is not None and prev_lastf > self.frames_written + self.buffer_limit:
                    self.past_would_force += 1
                return chunk[0].filled_count == self.px
            self.ts[r][off] = t
        else:
            self.ts[r][off] = prev_ts + t
        ts = self.ts[r][off]
        if max(ts - 1, 0) // self.tpf > prev_lastf:
            if d != D_EMPTY:
                if self.abs_t and self.view != VIEW_SAE:
                    t = max(t - (prev_ts & U32), 0)
                self.lasti[r][off] = get_frame_value(0, d, t, self.source, float(self.ref_interval), self.pdm,
                                                     self.delta_t_max, self.view, ts & U32, prev_ts & U32)
            self.lastf[r][off] = max(ts - 1, 0) // self.tpf
            a = self.lastf[r][off] - self.frame_idx_offsets[r]
            if a > 0:
                for _ in range(a):
                    chunk.append(_Frame(self.px))
                self.frame_idx_offsets[r] += a
            for i in range(prev_lastf, self.lastf[r][off]):
                idx = i - self.frames_written + 1
                if idx >= 0:
                    fr = chunk[idx]
                    if not fr.some[off]:
                        fr.some[off] = True
                        fr.val[off] = self.lasti[r][off]
                        fr.filled_count += 1
                else:
                    self.late_drops += 1
        if self.round_up and ts % self.ref_interval > 0:
            self.ts[r][off] = (ts // self.ref_interval + 1) * self.ref_interval
        if self.buffer_limit is not None:
            if self.lastf[r][off] > self.frames_written + self.buffer_limit:
                if chunk[0].filled_count < self.px:
                    self.row_forced[r] = True
                chunk[0].filled_count = self.px
        if chunk[0].filled_count > self.px:
            chunk[0].filled_count = self.px
        return chunk[0].filled_count == self.px

    def ingest_event(self, x, y, c, d, t):
        """Framer::ingest_event (driver.rs:437-562), detect_features off"""
        cc = 0 if c == 0xFF else c
        assert x < self.w and y < self.h and cc < self.ch
        was_forced = self.row_forced[y]
        self.chunk_filled[y] = self._chunk(y, x * self.ch + cc, d, t)
        self.n_ingested += 1
        filled = all(self.chunk_filled)
        if self.row_forced[y] and not was_forced and not filled:
            self.stalls += 1
        return filled

    def set_buffer_limit(self, buffer_limit):
        self.buffer_limit = buffer_limit
        self.limit_set = True

    def is_frame_0_filled(self):
        if self.buffer_limit is not None:
            for chunk in self.frames:
                if len(chunk) > self.buffer_limit:
                    return True
        return all(self.chunk_filled)

    def pop_next_frame(self):
        out = []
        for r in range(self.h):
            chunk = self.frames[r]
            out.append(chunk.popleft())
            if not chunk:
                chunk.append(_Frame(self.px))
                self.frame_idx_offsets[r] += 1
            self.chunk_filled[r] = chunk[0].filled_count == self.px
            self.row_forced[r] = False
        self.frames_written += 1
        return out

    def flush_frame_buffer(self):
        if any(len(chunk) > 1 for chunk in self.frames):
            for r in range(self.h):
                fr = self.frames[r][0]
                for i in range(self.px):
                    if not fr.some[i]:
                        fr.some[i] = True
                        fr.val[i] = self.lasti[r][i]
                        fr.filled_count += 1
                        self.lastf[r][i] += 1
                self.chunk_filled[r] = True
        else:
            self.chunk_filled[0] = False
        return self.is_frame_0_filled()

    # ---- adder.rs:339-356: the loop in front of the read loop ----
    def _show(self, returned=False):
        if returned:
            if any(self.row_forced):
                self.forced_pops += 1
            else:
                self.natural_pops += 1
        first = len(self.popped)
        while self.is_frame_0_filled():
            new_frame = self.pop_next_frame()
            val = np.concatenate([f.val for f in new_frame])
            some = np.concatenate([f.some for f in new_frame])
            self.running[some] = val[some]
            self.popped.append((self.n_ingested - 1, np.where(some, val, 0).astype(np.uint8), some,
                                self.running.copy()))
        self.longest_cascade = max(self.longest_cascade, len(self.popped) - first)

    def feed(self, events):
        """consume() over and over while events remain; a consume that returns at a full frame is followed at once by
        the next one (whose opening loop pops), the product's "pops happen right after the event"."""
        first = len(self.popped)
        if self.limit_set:  # adaptive_state_update came between two consume calls: the next one opens with its loop
            self._show()
            self.limit_set = False
        for ev in events:
            if self.ingest_event(int(ev["x"]), int(ev["y"]), int(ev["c"]), int(ev["d"]), int(ev["t"])):
                self._show(returned=True)
        return self.popped[first:]

    def finish(self):
        """the Err arm: flush_frame_buffer and the consume recursion alternate"""
        first = len(self.popped)
        if self.limit_set:
            self._show()
            self.limit_set = False
        while self.flush_frame_buffer():
            self.flushes += 1
            self._show()
        return self.popped[first:]


def unit_chain(events, width, channels, *, tpf, ref_interval, abs_t, round_up):
    """The per-unit clock of ingest_event_for_chunk alone, event by event in stream order: -> int32 arrays row, from,
    to, L (the unit's last_filled after the event; -1 for an AbsoluteT event from the unit's past), plus the unit of
    each event.  (from, to] is the event's fill range, empty when from == to.  The input of the product's schedule."""
    n = len(events)
    row, frm, to, last, unit = (np.zeros(n, np.int32) for _ in range(5))
    ts, lastf = {}, {}
    for i, ev in enumerate(events):
        x, y, c, t = int(ev["x"]), int(ev["y"]), int(ev["c"]), int(ev["t"])
        u = (y * width + x) * channels + (0 if c == 0xFF else c)
        pts, pl = ts.get(u, 0), lastf.get(u, -1)
        row[i], unit[i], frm[i], to[i] = y, u, pl, pl
        if abs_t and pts >= t:
            last[i] = -1
            continue
        cur = t if abs_t else pts + t
        q = max(cur - 1, 0) // tpf
        if q > pl:
            lastf[u] = to[i] = q
        last[i] = lastf.get(u, -1)
        if round_up and cur % ref_interval > 0:
            cur = (cur // ref_interval + 1) * ref_interval
        ts[u] = cur
    return row, frm, to, last, unit


def some_masks_from_schedule(pops, frm, to, unit, n_units):
    """The content rule of include/adder_viz_player.h: in the frame j popped after event P, unit u is Some iff the one
    event of u whose fill range contains j has index <= P.  -> bool [len(pops), n_units] (before any flush fill)."""
    out = np.zeros((len(pops), n_units), bool)
    for i in range(len(frm)):
        for j in range(int(frm[i]) + 1, int(to[i]) + 1):
            if j < len(pops) and i <= pops[j]:
                out[j, unit[i]] = True
    return out
