"""Literal pure-Python restatement of the video half of the reference's adder-to-dvs (adder-to-dvs/src/main.rs:189-239,
241-288, 382-411, 424-448) on top of tests/dvs_oracle.py -- the yardstick of the DVS event video and the event-count
map (include/adder_dvs.h).  It keeps a real collections.deque of [h][w] planes (the reference's frame is that plane
three times: set_instant_dvs_pixel writes one value into the three channels).

The reference never calls set_instant_dvs_pixel; the join restated here is the one of its sibling tool
(bin_cv/aedat4_dvs_visualize.rs:132-145, 203-206): at every fire point, value 255 for on, 0 for off, blank = 128.
draw=False is the reference as it stands: nothing is ever drawn.

Errors follow the library's rule (tests/dvs_oracle.py): a bad event stops the run, and nothing of it is applied -- it
is not counted either.

The census counts what a run met: pops with an empty deque (= frame indices skipped), late events dropped from the
video, pixels overwritten inside one frame, deques restarted at frame_count after running empty.
"""
import collections

import numpy as np

import dvs_oracle as R

BLANK = 128
U128_MAX = (1 << 128) - 1


def f32_as_u128(q):
    """Rust's `f32 as u128`: truncation, saturating, NaN -> 0."""
    q = np.float32(q)
    if np.isnan(q) or q <= 0:
        return 0
    if np.isinf(q):
        return U128_MAX
    return int(q)


def frame_length(tps, fps):
    with np.errstate(all="ignore"):
        return f32_as_u128(np.float32(tps) / np.float32(fps))  # (meta.tps as f32 / args.fps) as u128


def buffer_ticks(tps, buffer_secs):
    with np.errstate(all="ignore"):
        return f32_as_u128(np.float32(tps) * np.float32(buffer_secs))  # (meta.tps as f32 * args.buffer_secs) as u128


def count_byte(count, m):
    """((event_counts as f32 / max_px_event_count as f32) * 255.0) as u8, both u16"""
    with np.errstate(all="ignore"):
        v = (np.float32(count) / np.float32(m)) * np.float32(255.0)
    if np.isnan(v) or v <= 0:
        return 0
    return 255 if v >= 255 else int(v)


class DvsVideoRestatement:
    def __init__(self, meta, tps, fps=100.0, buffer_secs=10.0, draw=True, theta=0.01):
        self.dvs = R.DvsRestatement.from_meta(meta, theta)
        self.w, self.h, self.ch = meta["width"], meta["height"], meta["channels"]
        self.fps = np.float32(fps)
        self.draw = draw
        self.frame_length = frame_length(tps, fps)
        self.buffer = buffer_ticks(tps, buffer_secs)
        assert self.frame_length > 0  # the reference would divide by it
        self.event_counts = np.zeros((self.h, self.w, self.ch), np.uint16)
        self.max_px_event_count = 0
        self.deque = collections.deque([self.blank()])  # instantaneous_frame_deque
        self.frame_count = 0
        self.current_t = 0
        self.written = []  # (frame index, plane) in the order the reference writes them
        self.events_out = []
        self.bad = None  # the index of the bad event that ended the stream: its position's check was the last one
        self.census = collections.Counter()
        self._drawn = set()  # census only: (frame, y, x) drawn so far

    def blank(self):
        return np.full((self.h, self.w), BLANK, np.uint8)

    def check(self):
        """main.rs:214-239"""
        if self.current_t > self.frame_count * self.frame_length + self.buffer:
            if self.deque:
                self.written.append((self.frame_count, self.deque.popleft()))
                self.census["pops"] += 1
            else:
                self.census["empty_pops"] += 1
            self.frame_count += 1

    def set_instant_dvs_pixel(self, x, y, frame_idx, value):
        """main.rs:424-448"""
        grow_len = frame_idx - self.frame_count - len(self.deque) + 1
        if grow_len > 0 and not self.deque:
            self.census["restarts"] += 1
        for _ in range(grow_len):
            self.deque.append(self.blank())
        if frame_idx >= self.frame_count:
            if (frame_idx, y, x) in self._drawn:
                self.census["overwritten"] += 1
            self._drawn.add((frame_idx, y, x))
            self.census["drawn"] += 1
            self.deque[frame_idx - self.frame_count][y, x] = value
        else:
            self.census["late"] += 1

    def run(self, events):
        """-> the index of the bad event that stopped the run, or None.  May be called again with more events."""
        for k, ev in enumerate(events):
            self.check()
            x, y, c, d, t = (int(v) for v in ((ev["x"], ev["y"], ev["c"], ev["d"], ev["t"]) if hasattr(ev, "dtype")
                                              else ev))
            c = 0 if c == 0xFF else c
            first = (y, x, c) not in self.dvs.px  # `None =>` (main.rs:251): the event creates the unit's state
            out, bad = self.dvs.run([(x, y, c, d, t)])
            if bad is not None:  # the failing digest_event of main.rs:241: the check above was the loop's last
                self.bad = k
                return k
            self.event_counts[y, x, c] = (int(self.event_counts[y, x, c]) + 1) & 0xFFFF  # the release build wraps
            self.max_px_event_count = max(self.max_px_event_count, int(self.event_counts[y, x, c]))
            self.census["events"] += 1
            if first:
                continue
            self.current_t = max(self.dvs.px[(y, x, c)][2], self.current_t)
            for (ft, fx, fy, p) in out:
                self.events_out.append((ft, fx, fy, p))
                self.census["fired"] += 1
                if self.draw:
                    frame_idx = ft // self.frame_length  # ((old_t + 1) / frame_length) as usize
                    self.set_instant_dvs_pixel(fx, fy, frame_idx, 255 if p else 0)
        return None

    def finish(self):
        """main.rs:241 (the loop's last check comes before the failing digest_event), 382-411.  After a bad event
        that check has been made already, in front of the event that failed."""
        if self.bad is None:
            self.check()
        if not self.deque:
            self.deque.append(self.blank())
            self.census["blank_at_finish"] += 1
        k = 0
        while self.deque:
            self.written.append((self.frame_count + k, self.deque.popleft()))
            k += 1

    def count_map(self):
        """main.rs:386-394: a clone of a frame (128 everywhere), the stream's channels overwritten"""
        m = np.full((self.h, self.w, 3), BLANK, np.uint8)
        for y in range(self.h):
            for x in range(self.w):
                for c in range(self.ch):
                    m[y, x, c] = count_byte(int(self.event_counts[y, x, c]), self.max_px_event_count)
        return m

    def frames(self, rgb=False):
        """-> (frame indices, [n][h][w] planes ([n][h][w][3] with rgb))"""
        idx = [i for i, _ in self.written]
        planes = np.stack([f for _, f in self.written]) if self.written else np.zeros((0, self.h, self.w), np.uint8)
        return idx, (np.repeat(planes[..., None], 3, axis=-1) if rgb else planes)

    def times(self, playback_slowdown=1.0):
        """The timestamps of the written frames (main.rs:198-200, 226-233): current_frame_time / playback_slowdown,
        current_frame_time accumulating 1.0 / fps as f64."""
        frame_duration = 1.0 / float(self.fps)
        out, cur = [], 0.0
        for _ in self.written:
            out.append(cur / playback_slowdown)
            cur += frame_duration
        return out

    def skipped(self):
        """frame indices below the last written one that were never written"""
        idx = [i for i, _ in self.written]
        return (max(idx) + 1 - len(idx)) if idx else 0


def times_text(times):
    return "".join("%.9f\n" % t for t in times).encode()


def restate(meta, tps, events, finish=True, **kw):
    v = DvsVideoRestatement(meta, tps, **kw)
    v.run(events)
    if finish:
        v.finish()
    return v
