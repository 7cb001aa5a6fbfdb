"""Expected values of the transcoder's live view (Video::instantaneous_view_mode, display_frame_features), restated on
the committed CPU oracle -- not on the code under test.

Views: one oracle.Pixel per unit, stepped frame by frame with the context's parameters.  After each step node(0) gives
has_best / best_d / best_delta_t; running_t is the float32 running sum of the time steps; last_fired_t follows from the
unit's own emitted events (event_pixel_tree.rs:113-137, :257):
  AbsoluteT FramePerfect  the last event's t rounded up to a multiple of ref_time
  AbsoluteT Continuous    the last event's t
  DeltaT                  the t of the last D_EMPTY filler of a collapsed pop (its t is running_t before the step), else 0
The four formulas of <u8 as FrameValue>::get_frame_value (framer/scale_intensity.rs:54-104) are restated in numpy
float32 / float64 with Rust's `as` casts.

Features: handle_features (video.rs:893-918) is restated in Python over oracle_fast_is_feature on the VIEW plane: the
circular windows per row chunk, the tests c in {None, 0}, coord != next.coord and d != D_EMPTY, insert / remove, the
per-frame new set, the low c_thresh squares (:1089-1105) and the display frame as a literal scatter of draw_feature_coord
(utils/viz.rs:94-120).  test_live_view_cpu.py ties this file to oracle.Video in the Intensity view before anything is
compared with it.
"""
import ctypes as C
import math

import numpy as np

from oracle import oracle as O

VIEW_INTENSITY, VIEW_D, VIEW_DELTA_T, VIEW_SAE = 0, 1, 2, 3
SHOW_OFF, SHOW_INSTANT, SHOW_HOLD = 0, 1, 2
D_EMPTY = 255


def practical_d_max_exact(delta_t_max, ref_time):
    """log2(255 * (delta_t_max / ref_time)): integer division, f32 product, exact logarithm rounded to f32."""
    arg = np.float32(255.0) * np.float32(int(delta_t_max) // int(ref_time))
    return np.float32(math.log2(float(arg))) if arg > 0 else np.float32(-np.inf)


def as_u8(v):
    """Rust's float `as u8`: saturating, NaN -> 0."""
    v = np.asarray(v)
    out = np.zeros(v.shape, np.uint8)
    ok = v > 0  # (False for NaN)
    with np.errstate(invalid="ignore"):
        out[ok] = np.minimum(v[ok], 255.0).astype(np.uint8)
    return out


def view_value(view, d, t, running_u32, last_fired_u32, ref_time, delta_t_max, practical_d_max):
    """u8::get_frame_value, SourceType U8, elementwise over uint32 arrays (t = delta_t as u32)."""
    d = np.asarray(d, np.uint32)
    t = np.asarray(t, np.uint32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if view == VIEW_D:
            return as_u8(d.astype(np.float32) / np.float32(practical_d_max) * np.float32(255.0))
        if view == VIEW_DELTA_T:
            return as_u8(t.astype(np.float32) / np.float32(np.uint32(delta_t_max)) * np.float32(255.0))
        if view == VIEW_SAE:
            diff = (np.asarray(running_u32, np.uint32) - np.asarray(last_fired_u32, np.uint32)).astype(np.uint32)  # wraps
            return as_u8(diff.astype(np.float32) / np.float32(np.uint32(delta_t_max)) * np.float32(255.0))
        # Intensity: event_to_intensity (scale_intensity.rs:262-270) * tpf in f64; D_SHIFT[128] = 0, d > 128 -> 0
        shift = np.where(d < 128, np.ldexp(1.0, np.minimum(d, 127).astype(np.int32)), 0.0).astype(np.float64)
        inten = np.where(t == 0, shift, shift / np.maximum(t, 1).astype(np.float64))
        return as_u8(inten * np.float64(ref_time))


def f32_as_u32(v):
    """Rust's f32 `as u32`."""
    v = float(v)
    if not v > 0:
        return 0
    return min(int(v), 0xFFFFFFFF)


def draw_crosses(plane, coords):
    """draw_feature_coord for every (x, y) of coords, clipped to the plane (the product's features never need it)."""
    out = plane.copy()
    H, W, Cn = out.shape
    chans = [0] if Cn == 1 else [0, 1, 2]
    for x, y in coords:
        for i in range(-2, 3):
            if 0 <= y + i < H:
                out[y + i, x, chans] = 255
            if 0 <= x + i < W:
                out[y, x + i, chans] = 255
    return out


class LiveView:
    """The state of one Video<W> with a view mode and feature display, frame by frame."""

    def __init__(self, W, H, Cn=1, *, time_mode=O.ABSOLUTE_T, multi_mode=O.COLLAPSE, ref_time=255, delta_t_max=7650,
                 pixel_mode=O.FRAME_PERFECT, c_thresh_max=7, c_increase_velocity=7, view=VIEW_INTENSITY, practical_d_max=None,
                 detect=False, adjust=False, c_thresh_baseline=2, feature_c_radius=0, chunk_rows=1, show=SHOW_OFF):
        self.W, self.H, self.Cn = W, H, Cn
        self.time_mode, self.multi_mode, self.ref_time, self.dtm, self.mode = time_mode, multi_mode, ref_time, delta_t_max, pixel_mode
        self.c_max, self.vel = c_thresh_max, c_increase_velocity
        self.view, self.pdm = view, practical_d_max
        self.detect, self.adjust, self.baseline, self.radius = detect, adjust, c_thresh_baseline, feature_c_radius
        self.chunk_rows, self.show = chunk_rows, show
        self.L = O.lib()
        n = W * H * Cn
        self.px = []
        for u in range(n):
            y, r = divmod(u, W * Cn)
            x, c = divmod(r, Cn)
            p = O.Pixel(1.0, x, y, 0xFF if Cn == 1 else c)
            p.time_mode(time_mode)
            p.set_c_thresh(10, 1)
            self.px.append(p)
        self.cth = np.full(n, 10, np.uint8)   # PixelArena::new (event_pixel_tree.rs:82-83)
        self.ctr = np.full(n, 1, np.uint8)
        self.running_t = np.float32(0.0)
        self.last_fired = np.zeros(n, np.uint32)
        self.plane = np.zeros((H, W, Cn), np.uint8)
        # the same pixels seen through every view (valid while nothing feeds the plane back into the pixels: no
        # feature_rate_adjustment) -- one run of the pixels serves four comparisons
        self.planes = {v: np.zeros((H, W, Cn), np.uint8) for v in (VIEW_INTENSITY, VIEW_D, VIEW_DELTA_T, VIEW_SAE)}
        self.rt_px = np.zeros(n, np.float32)  # sparse steps: PixelArena::running_t per unit
        self.feature_set = np.zeros((H, W), np.uint8)
        self.new_features = []
        self.display = self.plane.copy()
        self.collapsed_pops = 0      # units that took the :257 path so far
        self.no_best = np.zeros(n, bool)   # units without a best event after the last frame

    def reset_c_thresh(self, baseline):
        self.cth[:] = baseline
        self.ctr[:] = 0
        for p in self.px:
            p.set_c_thresh(baseline, 0)

    def set_delta_t_max(self, dtm):
        self.dtm = dtm

    def set_view(self, view, practical_d_max=None):
        self.view, self.pdm = view, practical_d_max

    def _pdm(self):
        return practical_d_max_exact(self.dtm, self.ref_time) if self.pdm is None else np.float32(self.pdm)

    def _advance_counters(self, u, time):
        """arena_integrate's tail (event_pixel_tree.rs:399-411), for the counter the oracle does not hand out."""
        if self.cth[u] < self.c_max:
            if self.ctr[u] >= ((self.vel - 1) & 0xFF):
                self.cth[u] = min(int(self.cth[u]) + 1, 255)
                self.ctr[u] = 0
            else:
                inc = (f32_as_u32(time) // self.ref_time) & 0xFF
                self.ctr[u] = min(int(self.ctr[u]) + inc, 255)

    def _unit_events(self, u, p, rt_before_u32, popped_before):
        ev = p.events()
        if len(ev):
            self.L.oracle_px_clear_events(C.c_void_p(p.h))
            for i, e in enumerate(ev):
                t = int(e["t"])
                if self.time_mode == O.ABSOLUTE_T:
                    if self.mode == O.FRAME_PERFECT:
                        t = ((t + self.ref_time - 1) // self.ref_time) * self.ref_time
                    self.last_fired[u] = np.uint32(t & 0xFFFFFFFF)
                elif e["d"] == D_EMPTY and t == rt_before_u32 and popped_before and i > 0 and ev[i - 1]["d"] != D_EMPTY:
                    self.last_fired[u] = np.uint32(t)
                if e["d"] == D_EMPTY and t == rt_before_u32 and popped_before:
                    self.collapsed_pops += 1
        return ev

    def step(self, frame, time_spanned=None):
        """One integrate_matrix (video.rs:651-778): the frame's events in raster order."""
        T = np.float32(self.ref_time if time_spanned is None else time_spanned)
        frame = np.ascontiguousarray(frame, np.uint8).reshape(-1)
        rt_before = f32_as_u32(self.running_t)
        self.running_t = np.float32(self.running_t + T)
        rt_after = f32_as_u32(self.running_t)
        n = len(self.px)
        has = np.zeros(n, bool)
        bd = np.zeros(n, np.uint32)
        bt = np.zeros(n, np.uint32)
        events = []
        for u, p in enumerate(self.px):
            v = int(frame[u])
            popped = bool(self.L.oracle_px_popped_dtm(C.c_void_p(p.h)))
            p.step(v, float(T), self.mode, self.multi_mode, self.dtm, self.ref_time, self.c_max, self.vel)
            self._advance_counters(u, T)
            ev = self._unit_events(u, p, rt_before, popped)
            if len(ev):
                events.append(ev)
            nd = p.node(0)
            if nd["has_best"]:
                has[u], bd[u], bt[u] = True, nd["best_d"], f32_as_u32(nd["best_delta_t"])
        self.no_best = ~has
        self._write_planes(has, bd, bt, np.full(n, rt_after, np.uint32))
        events = np.concatenate(events) if events else np.zeros(0, O.EVENT_DTYPE)
        self._handle_features(events)
        return events

    def _write_planes(self, has, bd, bt, clock):
        for v, plane in list(self.planes.items()) + [(self.view, self.plane)]:
            vals = view_value(v, bd, bt, clock, self.last_fired, self.ref_time, self.dtm, self._pdm())
            plane.reshape(-1)[has] = vals[has]

    def step_sparse(self, steps):
        """adder_hip_integrate_sparse with intensity == frame_val and pad == 0: one integrate_for_px per step, the plane
        sampled after every step (prophesee.rs:259-283)."""
        n = len(self.px)
        events = []
        for st in steps:
            u = (int(st["y"]) * self.W + int(st["x"])) * self.Cn + (0 if self.Cn == 1 else int(st["c"]))
            p = self.px[u]
            T = np.float32(st["time"])
            rt_before = f32_as_u32(self.rt_px[u])
            popped = bool(self.L.oracle_px_popped_dtm(C.c_void_p(p.h)))
            p.step(int(st["frame_val"]), float(T), self.mode, self.multi_mode, self.dtm, self.ref_time, self.c_max, self.vel)
            self.rt_px[u] = np.float32(self.rt_px[u] + T)
            ev = self._unit_events(u, p, rt_before, popped)
            if len(ev):
                events.append(ev)
            nd = p.node(0)
            if nd["has_best"]:
                has = np.zeros(n, bool)
                has[u] = True
                bd = np.zeros(n, np.uint32)
                bt = np.zeros(n, np.uint32)
                bd[u], bt[u] = nd["best_d"], f32_as_u32(nd["best_delta_t"])
                clock = np.zeros(n, np.uint32)
                clock[u] = f32_as_u32(self.rt_px[u])
                self._write_planes(has, bd, bt, clock)
        return np.concatenate(events) if events else np.zeros(0, O.EVENT_DTYPE)

    def _handle_features(self, events):
        self.display = self.plane.copy()  # video.rs:742-744
        self.new_features = []
        if not self.detect:
            return
        img = np.ascontiguousarray(self.plane)
        chunk = events["y"].astype(np.int64) // self.chunk_rows
        for ch in np.unique(chunk):
            ev = events[chunk == ch]
            for i in range(len(ev)):
                e1, e2 = ev[i], ev[(i + 1) % len(ev)]
                same = e1["x"] == e2["x"] and e1["y"] == e2["y"] and e1["c"] == e2["c"]
                if e1["c"] in (0xFF, 0) and not same and e1["d"] != D_EMPTY:
                    x, y = int(e1["x"]), int(e1["y"])
                    if self.L.oracle_fast_is_feature(img.ctypes.data, self.W, self.H, self.Cn, x, y):
                        if not self.feature_set[y, x]:
                            self.feature_set[y, x] = 1
                            self.new_features.append((x, y))
                    else:
                        self.feature_set[y, x] = 0
        if self.show == SHOW_HOLD:
            ys, xs = np.nonzero(self.feature_set)
            self.display = draw_crosses(self.display, list(zip(xs.tolist(), ys.tolist())))
        elif self.show == SHOW_INSTANT:
            self.display = draw_crosses(self.display, self.new_features)
        if self.adjust and self.radius > 0:  # :1089-1105
            low = min(self.baseline, 2)
            r = self.radius
            for x, y in self.new_features:
                for row in range(max(y - r, 0), min(y + r, self.H - 1) + 1):
                    for col in range(max(x - r, 0), min(x + r, self.W - 1) + 1):
                        for c in range(self.Cn):
                            u = (row * self.W + col) * self.Cn + c
                            self.cth[u] = low
                            self.px[u].set_c_thresh(low, int(self.ctr[u]))

    def c_thresh_plane(self):
        return self.cth.reshape(self.H, self.W, self.Cn).copy()

    def check_c_thresh_against_pixels(self):
        got = np.array([self.L.oracle_px_c_thresh(C.c_void_p(p.h)) for p in self.px], np.uint8)
        return np.array_equal(got, self.cth)


def live_clip(W, H, Cn, frames, seed=O.SEED):
    """Scene content with the top-left quarter held static and the bottom-right quarter noise: quiet, firing and popped
    units all occur."""
    clip = O.synth_clip(O.CONTENT_SCENE, W, H, Cn, frames, seed=seed)
    noise = O.synth_clip(O.CONTENT_NOISE, W, H, Cn, frames, seed=seed)
    clip[:, : H // 2, : W // 2] = clip[0, : H // 2, : W // 2]
    clip[:, H // 2:, W // 2:] = noise[:, H // 2:, W // 2:]
    return clip
