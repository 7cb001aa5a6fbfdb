"""A literal restatement of the reference's Prophesee source (transcoder/source/prophesee.rs): parse_header,
decode_event, Prophesee::new / consume / end_events and the CLI's .crf(c), over the oracle's Continuous Video and
its sparse driver (integrate_for_px per step, in order).  f64 exp / ln_1p are libm's (math.exp, math.log1p).

It is the yardstick of tests/test_prophesee_cpu.py and tests/test_gpu_prophesee.py; the reference has no .dat
golden.  Where the reference panics, this raises: BadHeader, BadRecord(index), EndAssert.

Prophesee(.., census=c) also counts, per pixel, the arms of the chain a run takes (tests/chain_arms.py names them);
the events do not depend on it."""
import math

import numpy as np

from oracle import oracle as O

VIEW_INTERVAL = 1000000 // 60
# Crf rows 0..9 (rate_controller.rs): baseline C, max C, C increase velocity
CRF = ((0, 0, 10), (0, 1, 9), (1, 3, 8), (2, 7, 7), (5, 9, 6), (6, 10, 5), (7, 13, 4), (8, 16, 3), (10, 20, 2),
       (15, 25, 1))
M32 = 0xFFFFFFFF


class BadHeader(ValueError):
    pass


class BadRecord(ValueError):
    def __init__(self, index):
        super().__init__(f"record {index} is outside the plane")
        self.index = index


class EndAssert(AssertionError):
    pass


def _parse_u32(w):
    s = w.decode("utf-8")  # from_utf8(..).ok(): a bad word parses as None too
    if s.startswith("+"):
        s = s[1:]
    if not s or not s.isascii() or not s.isdigit():
        return None
    v = int(s)
    return v if v <= M32 else None


def parse_header(data):
    """:367-422 -> (bod, ev_type, ev_size, (height, width))."""
    pos, lines, size = 0, 0, [None, None]
    while True:
        if pos >= len(data) or data[pos] != ord("%"):
            break
        end = data.find(b"\n", pos)
        line = data[pos:] if end < 0 else data[pos:end + 1]
        words = [w for w in _split(line)]
        if len(words) > 1 and words[1] in (b"Height", b"Width"):
            if len(words) < 3 or len(words[2]) == 0:
                raise BadHeader("line_to_hw: unwrap on a missing word")
            w = words[2][:-1] if words[2].endswith(b"\n") else words[2]
            try:
                v = _parse_u32(w)
            except UnicodeDecodeError:
                v = None
            size[0 if words[1] == b"Height" else 1] = v
        lines += 1
        pos += len(line)
    ev_type = ev_size = 0
    if lines > 0:
        if pos + 2 > len(data):
            raise BadHeader("read_exact of the type bytes")
        ev_type, ev_size = data[pos], data[pos + 1]
        if ev_size != 8 or ev_type not in (0, 12):
            raise BadHeader("Invalid Prophesee event size")
        pos += 2
    h = 70 if size[0] is None else size[0]
    w = 100 if size[1] is None else size[1]
    return pos, ev_type, ev_size, (h, w)


def _split(line):
    out, cur = [], bytearray()
    for c in line:
        if c in (0x20, 0x09):
            out.append(bytes(cur))
            cur = bytearray()
        else:
            cur.append(c)
    out.append(bytes(cur))
    return out


def plane_of(h, w):
    """PlaneSize::new(width as u16, height as u16, 1)."""
    w16, h16 = w & 0xFFFF, h & 0xFFFF
    if w16 == 0 or h16 == 0:
        raise BadHeader("PlaneSize::new refuses 0")
    return w16, h16


def decode_event(rec):
    """:437-452 over one 8-byte record."""
    t = int.from_bytes(rec[0:4], "little")
    data = int.from_bytes(rec[4:8], "little", signed=True)
    x = data & 0x3FF
    y = (data & 0xFFFC000) >> 14
    p = (data & 0x10000000) >> 28
    return t, x, y, p


def _as_u8(v):
    return 0 if not v > 0.0 else (255 if v >= 255.0 else int(v))


def _step(x, y, val, intensity, time, no_side):
    return (x, y, 0xFF, _as_u8(val), no_side, np.float32(intensity), np.float32(time))


class Prophesee:
    """Prophesee::new(ref_time, ..)[.crf(c)] over decoded records; run() = consume() until the input ends."""

    def __init__(self, width, height, ref_time, crf=None, census=None):
        self.W, self.H, self.ref_time = width, height, ref_time
        self.census = census
        # census only: a pixel's running time as its arena adds it up in f32 (the two start-up frames first)
        self.acc_t = [np.float32(2 * ref_time)] * (width * height) if census is not None else None
        v = O.Video(width, height, 1, time_mode=O.ABSOLUTE_T, multi_mode=O.COLLAPSE, ref_time=ref_time,
                    delta_t_max=2 * ref_time)
        v.set_pixel_mode(1)
        v.ensure_capacity(40)
        q = 3 if crf is None else crf
        v.set_crf_parameters(CRF[q][1], CRF[q][2])  # Crf::new(None) is quality 3
        if crf is not None:
            v.reset_c_thresh(CRF[crf][0])  # update_crf: every pixel's c_thresh to the baseline
        self.v = v
        self.last_t = [2] * (width * height)
        self.last_ln = [math.log1p(128.0 / 255.0)] * (width * height)
        self.running_t = 0
        self.theta = 0.02
        self.calls = []  # the events of every consume() that returned
        self.start_events = None
        self.end = None  # end_events' events

    def run(self, recs):
        """recs: a sequence of (t, x, y, p).  -> every event in order (start-up, groups, end)."""
        pos, n = 0, len(recs)
        while True:
            if self.running_t == 0:  # :117-133
                start = np.full((self.H, self.W, 1), 128, np.uint8)
                a = self.v.integrate_matrix(start, time_spanned=float(self.ref_time))
                b = self.v.integrate_matrix(start, time_spanned=float(self.ref_time))
                assert len(b) == self.W * self.H
                self.start_events = np.concatenate([a, b])
                self.running_t = 2
            batch, start_t = [], self.running_t
            while True:
                if pos >= n:
                    self.end = self.end_events()
                    return np.concatenate([self.start_events] + self.calls + [self.end])
                t, x, y, p = recs[pos]
                pos += 1
                if t > self.running_t:
                    self.running_t = t
                batch.append((pos - 1, t, x, y, p))
                if t > ((start_t + VIEW_INTERVAL) & M32):
                    break
            self.calls.append(self.consume_batch(batch))

    def consume_batch(self, batch):
        """:172-258 for one group."""
        steps, W, rt, cen = [], self.W, self.ref_time, getattr(self, "census", None)
        for idx, t, x, y, p in batch:
            if x >= W or y >= self.H:
                raise BadRecord(idx)  # ndarray indexing panics
            px = y * W + x
            last_t = self.last_t[px]
            if t < last_t:
                if cen is not None:
                    cen.hit("skip", px)
                continue
            ln = self.last_ln[px]
            if t > ((last_t + 1) & M32):
                val = (math.exp(ln) - 1.0) * 255.0
                if cen is not None:
                    cen.hit("gap", px)
                    if val > 255.0:
                        cen.hit("gap_clamp_hi", px)
                    elif val < 0.0:
                        cen.hit("gap_clamp_lo", px)
                if val < 0.0 or val > 255.0:  # mid_clamp_u8
                    val, ln = 128.0, math.log1p(128.0 / 255.0)
                gap = (t - last_t - 1) & M32
                if cen is not None:
                    if gap * rt > M32:
                        cen.hit("gap_time_wrap", px)
                    self._note_time(px, (gap * rt) & M32)
                steps.append(_step(x, y, val, val * float(gap), (gap * rt) & M32, 1))
            elif cen is not None:
                cen.hit("same_t" if t == last_t else "step_no_gap", px)
            new_ln = ln - self.theta if p == 0 else ln + self.theta
            self.last_ln[px] = new_ln
            self.last_t[px] = t
            if t > last_t:
                val = (math.exp(new_ln) - 1.0) * 255.0
                if cen is not None:
                    if val > 255.0:
                        cen.hit("step_clamp_hi", px)
                    elif val < 0.0:
                        cen.hit("step_clamp_lo", px)
                    self._note_time(px, rt)
                if val < 0.0 or val > 255.0:
                    val, new_ln = 128.0, math.log1p(128.0 / 255.0)
                self.last_ln[px] = new_ln
                steps.append(_step(x, y, val, val, rt, 0))
        if not steps:
            return np.zeros(0, O.EVENT_DTYPE)
        return self.v.integrate_sparse(np.array(steps, O.SPARSE_STEP_DTYPE))

    def end_events(self):
        """:325-365, raster order, no clamp."""
        steps, cen = [], getattr(self, "census", None)
        for y in range(self.H):
            for x in range(self.W):
                px = y * self.W + x
                val = (math.exp(self.last_ln[px]) - 1.0) * 255.0
                d = (self.running_t - self.last_t[px]) & M32
                if not d > 0:
                    raise EndAssert("assert!(running_t - dvs_last_timestamps > 0)")
                span = (d * self.ref_time) & M32
                if cen is not None:
                    if d * self.ref_time > M32:
                        cen.hit("end_span_wrap", px)
                    self._note_time(px, span)
                steps.append(_step(x, y, val, val * float(span), span, 1))
        return self.v.integrate_sparse(np.array(steps, O.SPARSE_STEP_DTYPE))

    def _note_time(self, px, time):
        """census only: a step of `time` ticks on px; counts the steps and pixels past f32's exact range and 2^31"""
        acc = self.acc_t[px] = np.float32(self.acc_t[px] + np.float32(time))
        for arm, limit in (("t_over_2p24", 1 << 24), ("t_over_2p31", 1 << 31)):
            if time > limit or acc > limit:
                self.census.hit(arm, px)

    def running_intensities(self):
        return self.v.running_intensities()[:, :, 0]


def decode_body(body):
    n = len(body) // 8
    r = np.frombuffer(bytes(body[: n * 8]), np.dtype([("t", "<u4"), ("d", "<i4")]))
    d = r["d"].astype(np.int64)
    return list(zip(r["t"].astype(np.int64).tolist(), (d & 0x3FF).tolist(), ((d & 0xFFFC000) >> 14).tolist(),
                    ((d & 0x10000000) >> 28).tolist()))


def transcode(dat, ref_time=1, crf=None):
    """A whole .dat file (bytes) -> (Prophesee after the run, every event in order)."""
    bod, _, _, (h, w) = parse_header(dat)
    W, H = plane_of(h, w)
    src = Prophesee(W, H, ref_time, crf)
    ev = src.run(decode_body(dat[bod:]))
    return src, ev
