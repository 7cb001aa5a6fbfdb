"""A literal Python restatement of the DAVIS chain (davis.rs:233-897 as the C++ mirror's Davis has it) over the
oracle's Video and its sparse driver: per packet the steps of each phase, the state planes and the events; on request
a census of the arms the packets reached.  Test infrastructure: the product never imports it."""
import math

import numpy as np

from oracle import oracle as O

FRAMED, RAW_DAVIS, RAW_DVS = 0, 1, 2
EVENT_DTYPE = np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("on", "u1"), ("pad", "u1", (3,))])
CRF = [(0, 0, 10), (0, 1, 9), (1, 3, 8), (2, 7, 7), (5, 9, 6), (6, 10, 5), (7, 13, 4), (8, 16, 3), (10, 20, 2), (15, 25, 1)]
NO_SIDE, INTEGRATE_ONLY, TEST_ONLY, FLUSH = 1, 2, 4, 8

# every arm of the chain.  The second check has two forms in integrate_dvs_events' signature -- t > ts2 (the only one
# consume() uses) and t < ts2 -- and the first fails in two ways, t below ts2 and t equal to it: all three are arms
ARMS = ("check1_skip", "check2_skip_below", "check2_skip_equal", "check2_skip_before_form", "first_ts_skip",
        "negative_ticks_skip", "on", "off", "event_clamp_low", "event_clamp_high", "gap_clamp_low", "gap_clamp_high", "gap_skip_after_clamp",
        "gap_skip_no_ts", "gap_skip_no_ticks", "round_tie_up", "round_tie_down", "saturate_0", "saturate_255")

f32 = np.float32


def events(t, x, y, on):
    ev = np.zeros(len(t), EVENT_DTYPE)
    ev["t"], ev["x"], ev["y"], ev["on"] = t, x, y, on
    return ev


def as_u8(v):
    return 0 if not v > 0.0 else (255 if v >= 255.0 else int(v))


def _hit(census, arm):
    if census is not None:
        census[arm] = census.get(arm, 0) + 1


def _steps(rows):
    return np.array(rows, O.SPARSE_STEP_DTYPE) if rows else np.zeros(0, O.SPARSE_STEP_DTYPE)


def dvs_steps(W, H, last_ts, last_ln, evs, ts1, ts2, c, tps, ref_time, census=None, after2=True):
    """integrate_dvs_events (davis.rs:233-466): the planes (flat, updated in place) -> the steps in step order.
    ts2 None: no second check; else the event must have t > ts2 (after2) or t < ts2."""
    tpm = f32(tps) / f32(1e6)
    rows = []
    for chunk in range(4):
        for e in evs:
            x, y, t = int(e["x"]), int(e["y"]), int(e["t"])
            assert x < W and y < H
            if y // (H // 4) != chunk:
                continue
            if not t < ts1:
                _hit(census, "check1_skip")
                continue
            if ts2 is not None and after2 and not t > ts2:
                _hit(census, "check2_skip_equal" if t == ts2 else "check2_skip_below")
                continue
            if ts2 is not None and not after2 and not t < ts2:
                _hit(census, "check2_skip_before_form")
                continue
            p = y * W + x
            last_val = (math.exp(last_ln[p]) - 1.0) * 255.0
            dmicro = t - int(last_ts[p])
            if dmicro == t:
                _hit(census, "first_ts_skip")
                continue
            dticks = f32(dmicro) * tpm
            if dticks < 0:
                _hit(census, "negative_ticks_skip")
                continue
            first = max(f32(f32(last_val) / f32(ref_time)) * dticks, f32(0.0))
            rows.append((x, y, 0xFF, 0, NO_SIDE | INTEGRATE_ONLY, f32(first), f32(dticks)))
            _hit(census, "on" if e["on"] else "off")
            last_ln[p] *= math.exp(c if e["on"] else -c)
            fv = (math.exp(last_ln[p]) - 1.0) * 255.0
            if fv <= 0.0:
                fv, last_ln[p] = 0.0, math.log1p(0.0)
                _hit(census, "event_clamp_low")
            elif fv > 255.0:
                fv, last_ln[p] = 255.0, math.log1p(1.0)
                _hit(census, "event_clamp_high")
            rows.append((x, y, 0xFF, as_u8(fv), NO_SIDE | TEST_ONLY, f32(fv), f32(0.0)))
            last_ts[p] = t
    return _steps(rows)


def gap_steps(W, H, last_ts, last_ln, start, tps, ref_time, census=None):
    """integrate_frame_gaps (davis.rs:468-598): raster order; the clamp rewrites last_ln before the skips."""
    tpm = f32(tps) / f32(1e6)
    rows = []
    for p in range(W * H):
        lv = (math.exp(last_ln[p]) - 1.0) * 255.0
        clamped = False
        if lv <= 0.0:
            lv, last_ln[p], clamped = 0.0, math.log1p(0.0), True
            _hit(census, "gap_clamp_low")
        elif lv > 255.0:
            lv, last_ln[p], clamped = 255.0, math.log1p(1.0), True
            _hit(census, "gap_clamp_high")
        dmicro = start - int(last_ts[p])
        skipped = None
        if dmicro == start:
            skipped = "gap_skip_no_ts"
        else:
            dticks = f32(dmicro) * tpm
            if dticks <= 0:
                skipped = "gap_skip_no_ticks"
        if skipped:
            _hit(census, skipped)
            if clamped:
                _hit(census, "gap_skip_after_clamp")
            continue
        integ = max((lv / float(ref_time)) * float(dticks), 0.0)
        rows.append((p % W, p // W, 0xFF, as_u8(lv), 0, f32(integ), f32(dticks)))
    return _steps(rows)


def frame_image(frame, mode, census=None):
    """convert_to(CV_8U, 255.0): saturate(round half to even(frame * 255)); zeros in RawDvs."""
    if mode == RAW_DVS:
        return np.zeros(frame.shape, np.uint8)
    prod = np.asarray(frame, np.float64) * 255.0
    r = np.rint(prod)
    if census is not None:
        fl = np.floor(prod)
        tie = (prod - fl) == 0.5
        for arm, m in (("round_tie_up", tie & (fl % 2 == 1)), ("round_tie_down", tie & (fl % 2 == 0)),
                       ("saturate_0", r < 0), ("saturate_255", r > 255)):
            if m.any():
                census[arm] = census.get(arm, 0) + int(m.sum())
    return np.clip(r, 0, 255).astype(np.uint8)


def frame_span(mode, start, end, ref_time):
    return f32(end - start) if mode == RAW_DAVIS else (f32(0.0) if mode == RAW_DVS else f32(ref_time))


class DavisOracle:
    """Davis::new + time_parameters(tps, ref_time, dtm, AbsoluteT) [+ crf]; push(packet) is one consume() with a cached
    packet, finish() the end of input."""

    def __init__(self, W, H, mode, *, tps, ref_time, dtm, crf=None, census=None):
        assert H % 4 == 0
        self.W, self.H, self.mode, self.tps, self.ref_time = W, H, mode, tps, ref_time
        self.census = census
        v = O.Video(W, H, 1, time_mode=O.ABSOLUTE_T, multi_mode=O.COLLAPSE, ref_time=ref_time, delta_t_max=dtm,
                    chunk_rows=H // 4)
        if mode != FRAMED:
            v.set_pixel_mode(1)
        v.ensure_capacity(40)
        if crf is not None:
            base, cmax, vel = CRF[crf]
            v.set_crf_parameters(cmax, vel)
            v.reset_c_thresh(base)
        else:
            v.set_crf_parameters(7, 7)
        self.v = v
        self.last_ts = np.zeros(W * H, np.int64)
        self.last_ln = np.zeros(W * H, np.float64)
        self.last_after, self.end_of_last = None, None

    def _run(self, steps):
        return self.v.integrate_sparse(steps) if len(steps) else np.zeros(0, O.EVENT_DTYPE)

    def push(self, pk):
        """-> dict(steps={phase: steps}, events, frame_events, last_ts, last_ln, image)"""
        W, H, mode = self.W, self.H, self.mode
        raw = mode != FRAMED
        frame = np.asarray(pk["frame"], np.float64).reshape(H, W)
        steps, ev = {}, []
        start, end = 0, self.ref_time
        if raw:
            start, end, c = int(pk["start"]), int(pk["end"]), float(pk["c"])
            if mode == RAW_DVS:
                end = start + 1
            held = self.last_after if self.last_after is not None else np.zeros(0, EVENT_DTYPE)
            steps["last_after"] = dvs_steps(W, H, self.last_ts, self.last_ln, held, start,
                                            self.end_of_last if mode != RAW_DVS else None, c, self.tps, self.ref_time,
                                            self.census)
            ev.append(self._run(steps["last_after"]))
            steps["before"] = dvs_steps(W, H, self.last_ts, self.last_ln, pk["before"], start, None, c, self.tps,
                                        self.ref_time, self.census)
            ev.append(self._run(steps["before"]))
            steps["gaps"] = gap_steps(W, H, self.last_ts, self.last_ln, start, self.tps, self.ref_time, self.census)
            ev.append(self._run(steps["gaps"]))
        img = frame_image(frame, mode, self.census)
        span = frame_span(mode, start, end, self.ref_time)
        if raw:
            steps["frame"] = _steps([(p % W, p // W, 0xFF, int(img.flat[p]), 0, f32(img.flat[p]), span)
                                     for p in range(W * H)])
            fe = self._run(steps["frame"])
        else:
            fe = self.v.integrate_matrix(img.reshape(H, W, 1), time_spanned=float(span))
        ev.append(fe)
        self.last_ln[:] = math.log1p(0.5) if mode == RAW_DVS else np.array([math.log1p(x) for x in frame.reshape(-1)])
        if raw:
            self.last_after, self.end_of_last = np.array(pk["after"], EVENT_DTYPE), end
            self.last_ts[:] = end
        return dict(steps=steps, events=np.concatenate(ev), frame_events=len(fe), image=img,
                    last_ts=self.last_ts.reshape(H, W).copy(), last_ln=self.last_ln.reshape(H, W).copy())

    def finish(self):
        if self.mode == FRAMED:
            return np.zeros(0, O.EVENT_DTYPE)
        W = self.W
        return self._run(_steps([(p % W, p // W, 0xFF, 0, NO_SIDE | FLUSH, f32(0.0), f32(0.0))
                                 for p in range(W * self.H)]))


def run(packets, W, H, mode, *, tps, ref_time, dtm, crf=None, census=None):
    """Every packet and the finish -> (list of push results, finish events, all events in order)."""
    d = DavisOracle(W, H, mode, tps=tps, ref_time=ref_time, dtm=dtm, crf=crf, census=census)
    res = [d.push(pk) for pk in packets]
    fin = d.finish()
    return res, fin, np.concatenate([r["events"] for r in res] + [fin])
