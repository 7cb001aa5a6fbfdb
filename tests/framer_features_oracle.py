"""Python restatement of Framer::ingest_event with detect_features on (adder-codec-rs/src/framer/driver.rs:437-553,
984-1133), FrameSequence::pop_features (:851-873) and get_running_intensities (:846-848) -- test helper.

Independent of the product: Python ints for BigT, its own per-unit chain (ingest_event_for_chunk restated here, every
get_frame_value arm of scale_intensity.rs:54-209), one mutable plane walked serially, the FeatureInterval deque.  The
corner test is the literal FAST of the CPU checker (oracle_fast_is_feature: utils/cv.rs:56-212 line by line), called
per candidate as tests/test_features.py's oracle_fast_plane calls it per pixel.

`Restatement.ingest(events)` adds what include/adder_framer.h defines around the reference's per-event function: the
player's `last_event` carried from call to call by calls made with detection on, features of the last call with their
index in the call's array, and the two places where the reference would panic or grow without bound (DequeBroken).
"""
import collections

import numpy as np

from oracle import oracle as O

EVENT_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("c", "u1"), ("d", "u1"), ("pad", "<u2"), ("t", "<u4")])
FEATURE_DTYPE = np.dtype([("index", "<u8"), ("t", "<u4"), ("x", "<u2"), ("y", "<u2")])
D_EMPTY = 255
DELTA_T, ABSOLUTE_T = 0, 1
VIEW_INTENSITY, VIEW_D, VIEW_DELTA_T, VIEW_SAE = 0, 1, 2, 3
U32 = 0xFFFFFFFF
f32 = np.float32


class DequeBroken(Exception):
    """features[idx] past the deque (the reference panics), or growth by more than 2^22 intervals (our limit)."""


def make_events(rows):
    """rows of (x, y, c, d, t); c None -> 0xFF"""
    ev = np.zeros(len(rows), EVENT_DTYPE)
    for i, (x, y, c, d, t) in enumerate(rows):
        ev[i] = (x, y, 0xFF if c is None else c, d, 0, t)
    return ev


def _as_uint(v, vmax):
    """Rust's float `as uN`: saturating, NaN -> 0"""
    v = float(v)
    if not v > 0.0:
        return 0
    if v >= vmax:
        return int(vmax)
    return int(v)


def event_to_intensity(d, t):  # scale_intensity.rs:262-270
    if d >= 129:
        return 0.0
    shift = 0.0 if d == 128 else float(2 ** d)
    return shift if t == 0 else shift / float(t)


def get_frame_value(value_type, d, t, source, tpf, practical_d_max, delta_t_max, view, running_t, last_fired_t):
    """<u8 / u16 / u32 as FrameValue>::get_frame_value (scale_intensity.rs:54-209)"""
    tmax = (255.0, 65535.0, 4294967295.0)[value_type]
    tmax_f32 = (f32(255.0), f32(65535.0), f32(4294967296.0))[value_type]  # u32::MAX as f32 rounds up
    if view == VIEW_D:
        return _as_uint(f32(d) / f32(practical_d_max) * tmax_f32, tmax)
    if view == VIEW_DELTA_T:
        return _as_uint(f32(t) / f32(delta_t_max) * tmax_f32, tmax)
    if view == VIEW_SAE:
        assert value_type == 0, "todo!() in the reference"
        return _as_uint(f32((running_t - last_fired_t) & U32) / f32(delta_t_max) * tmax_f32, tmax)
    intensity = event_to_intensity(d, t)
    if source == value_type:
        return _as_uint(intensity * tpf, tmax)
    smax = (255.0, 65535.0, 4294967295.0, 18446744073709551615.0)[source]
    return _as_uint(intensity / smax * tpf * tmax, tmax)


class Restatement:
    def __init__(self, width, height, channels=1, *, tps, ref_interval, delta_t_max, output_fps=None, codec_version=1,
                 time_mode=DELTA_T, source_camera=0, view_mode=0, source_type=0, practical_d_max=0.0, value_type=0):
        self.w, self.h, self.ch = width, height, channels
        self.ref_interval, self.delta_t_max = ref_interval, delta_t_max
        self.tpf = ref_interval
        if output_fps is not None:  # (tps as f32 / fps) as u32 (driver.rs:357-361)
            self.tpf = _as_uint(f32(tps) / f32(output_fps), 4294967295.0)
        self.abs_t = codec_version >= 2 and time_mode == ABSOLUTE_T
        self.round_up = codec_version >= 1 and source_camera <= 5
        self.view, self.source, self.pdm, self.vt = view_mode, source_type, practical_d_max, value_type
        n = width * height * channels
        self.ts = [0] * n           # pixel_ts_tracker (BigT)
        self.lastf = [-1] * n       # last_filled_tracker
        self.lasti = [0] * n        # last_frame_intensity_tracker
        self.frames = {}            # frame index -> (values, has) over units
        self.frames_written = 0
        self.detect = False
        self.running = np.zeros((height, width, channels), np.uint8)
        self.features = collections.deque()  # [end_ts, [(x, y)]]
        self.broken = None
        self.last = None            # carried last_event.t (None: no last event)
        self.last_features = np.zeros(0, FEATURE_DTYPE)
        self._L = O.lib()

    # ---- ingest_event_for_chunk (driver.rs:984-1133); returns the event's t as it is left ----
    def _chunk(self, u, d, t):
        prev_lastf, prev_ts = self.lastf[u], self.ts[u]
        if self.abs_t:
            if prev_ts >= t:
                return t
            self.ts[u] = t
        else:
            self.ts[u] = prev_ts + t
        ts = self.ts[u]
        q = max(ts - 1, 0) // self.tpf
        if q > prev_lastf:
            if d != D_EMPTY:
                if self.abs_t and self.view != VIEW_SAE:
                    t = max(t - (prev_ts & U32), 0)  # event.t.saturating_sub(prev_running_ts as u32)
                self.lasti[u] = get_frame_value(self.vt, d, t, self.source, float(self.ref_interval), self.pdm,
                                                self.delta_t_max, self.view, ts & U32, prev_ts & U32)
            self.lastf[u] = q
            for i in range(prev_lastf, q):
                if i - self.frames_written + 1 >= 0:
                    fr = self.frames.get(i + 1)
                    if fr is None:
                        n = len(self.ts)
                        fr = self.frames[i + 1] = (np.zeros(n, np.uint32), np.zeros(n, bool))
                    if not fr[1][u]:
                        fr[0][u] = self.lasti[u]
                        fr[1][u] = True
        if self.round_up and ts % self.ref_interval > 0:
            self.ts[u] = (ts // self.ref_interval + 1) * self.ref_interval
        return t

    def _is_feature(self, x, y, c):
        # is_feature(event.coord, plane, running_intensities): border 3, channel 0 / None, the literal scan
        if c not in (0, 0xFF):
            return False
        return bool(self._L.oracle_fast_is_feature(self.running.ctypes.data, self.w, self.h, self.ch, x, y))

    def _file(self, time, x, y):
        """driver.rs:497-549"""
        if self.broken:
            return
        tpf, fw, dq = self.tpf, self.frames_written, self.features
        idx = ((time // tpf) - (fw & U32)) & U32 if time // tpf >= fw else 0
        if time % tpf == 0 and idx > 0:
            idx -= 1
        if idx >= len(dq):
            if not dq:
                dq.append([tpf, []])
                dq.append([tpf * 2, []])
            new_end_ts = time if time % tpf == 0 else ((time // tpf + 1) * tpf) & U32  # u32, as a release build wraps
            running_end_ts = dq[-1][0] + tpf
            if running_end_ts <= new_end_ts and (new_end_ts - running_end_ts) // tpf >= 1 << 22:
                self.broken = "growth"
                return
            while running_end_ts <= new_end_ts:
                dq.append([running_end_ts, []])
                running_end_ts += tpf
        if idx >= len(dq):
            self.broken = "panic"
            return
        if dq[idx][0] < time:
            dq[idx][0] = time
        dq[idx][1].append((x, y))

    def ingest_event(self, ev, last_t):
        """Framer::ingest_event(&mut event, last_event) (driver.rs:437-553); ev = (x, y, c, d, t), last_t = last.t or None.
        Returns (t left in the event, whether a feature was filed for it)."""
        x, y, c, d, t = ev
        cc = 0 if c == 0xFF else c
        assert x < self.w and y < self.h and cc < self.ch
        u = (y * self.w + x) * self.ch + cc
        time = t
        t = self._chunk(u, d, t)
        found = False
        if self.detect:
            self.running[y, x, cc] = min(self.lasti[u], 255)  # Into<f64> then `as u8`: saturates
            if last_t is not None and time != last_t:
                if self._is_feature(x, y, c):
                    found = True
                    self._file(time, x, y)
        return t, found

    # ---- the call-level rules of include/adder_framer.h ----
    def detect_features(self, on):
        self.detect = bool(on)

    def reset_last_event(self):
        self.last = None

    def ingest(self, events, index_base=0):
        feats = []
        for i, e in enumerate(np.asarray(events, EVENT_DTYPE).tolist()):
            x, y, c, d, _, t = e
            t_after, found = self.ingest_event((x, y, c, d, t), self.last if self.detect else None)
            if self.detect:
                self.last = t_after
                if found:
                    feats.append((index_base + i, t, x, y))
        self.last_features = np.array(feats, FEATURE_DTYPE) if feats else np.zeros(0, FEATURE_DTYPE)
        return self.last_features

    def running_intensities(self):
        return self.running.copy()

    def pop_features(self):
        """driver.rs:851-873 -> (end_ts, [n][2] u16)"""
        if self.broken:
            raise DequeBroken(self.broken)
        dq = self.features
        if not dq:
            dq.append([self.tpf, []])
            dq.append([self.tpf * 2, []])
        else:
            dq.append([self.tpf + dq[-1][0], []])
        end_ts, coords = dq.popleft()
        return end_ts, np.array(coords, np.uint16).reshape(-1, 2)

    def frames_ready(self):
        n = 0
        while True:
            fr = self.frames.get(self.frames_written + n)
            if fr is None or not fr[1].all():
                return n
            n += 1

    def write_frame_bytes(self):
        """write_frame_bytes: frame 0 whether or not it is complete, pixels without a value read 0 (driver.rs:935-981)"""
        fr = self.frames.pop(self.frames_written, None)
        n = len(self.ts)
        vals = np.zeros(n, np.uint32) if fr is None else np.where(fr[1], fr[0], 0)
        self.frames_written += 1
        return vals.astype((">u1", ">u2", ">u4")[self.vt]).tobytes()

    def pop(self):
        """write_multi_frame_bytes: every complete frame, big-endian elements of 1 << value_type bytes"""
        out = []
        while True:
            fr = self.frames.get(self.frames_written)
            if fr is None or not fr[1].all():
                break
            out.append(fr[0].astype((">u1", ">u2", ">u4")[self.vt]).tobytes())
            del self.frames[self.frames_written]
            self.frames_written += 1
        return b"".join(out)


# Video::update_crf's table (rate_controller.rs:5-18): crf -> (c_thresh_baseline, c_thresh_max, c_increase_velocity)
CRF = [(0, 0, 10), (0, 1, 9), (1, 3, 8), (2, 7, 7), (5, 9, 6), (6, 10, 5), (7, 13, 4), (8, 16, 3), (10, 20, 2), (15, 25, 1)]


def transcode(clip, *, time_mode, multi_mode, crf, delta_t_max=7650):
    """Per-frame event arrays of the transcode checker for clip [T][H][W][C] at CRF quality `crf`."""
    T, H, W, Cn = clip.shape
    ov = O.Video(W, H, Cn, time_mode=time_mode, multi_mode=multi_mode, ref_time=255, delta_t_max=delta_t_max)
    ov.ensure_capacity(48)
    base, cmax, vel = CRF[crf]
    ov.set_crf_parameters(cmax, vel)
    ov.reset_c_thresh(base)
    return [ov.integrate_matrix(clip[k]) for k in range(T)]
