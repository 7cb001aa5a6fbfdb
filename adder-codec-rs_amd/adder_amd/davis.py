"""HipDavis: ctypes binding of the DAVIS -> ADDER transcoder in libadder_hip.so (include/adder_davis.h), the chain's
CPU forms (steps_host, gaps_host, frame_host), and davis_to_adder / davis_to_adder_file over in-memory EDI output.

A packet is what the EDI reconstructor hands to Davis::consume: a dict {frame [h, w] f64, c, start, end, before, after}
with the DVS events as DAVIS_EVENT_DTYPE arrays.  Frames and events are numpy arrays (host forms of the C-ABI) or
CUDA tensors (device forms: a float64 frame, uint8 tensors of whole 16-byte events).  Events come back as EVENT_DTYPE
arrays (host) or uint8 CUDA tensors of whole AdderEvents (device).
"""
import ctypes as C

import numpy as np

from . import _native as N

ABI_VERSION = 1
E_BAD_EVENT, E_ORDER = -22, -23
NO_CRF = -1
NO_BAD_EVENT = (1 << 64) - 1
FRAMED, RAW_DAVIS, RAW_DVS = 0, 1, 2
SOURCE_CAMERA_DAVIS_U8 = 7  # SourceCamera::DavisU8
CODEC_VERSION = 3

DAVIS_EVENT_DTYPE = np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("on", "u1"), ("pad", "u1", (3,))])
assert DAVIS_EVENT_DTYPE.itemsize == 16


class AdderDavisMeta(C.Structure):
    """include/adder_davis.h::AdderDavisMeta"""
    _fields_ = [("c", C.c_double), ("img_start_ts", C.c_int64), ("img_end_ts", C.c_int64), ("has_events", C.c_uint32),
                ("reserved0", C.c_uint32)]


class AdderDavisParams(C.Structure):
    """include/adder_davis.h::AdderDavisParams"""
    _fields_ = [("abi_version", C.c_uint32), ("width", C.c_uint16), ("height", C.c_uint16), ("mode", C.c_int32),
                ("tps", C.c_uint32), ("ref_time", C.c_uint32), ("delta_t_max", C.c_uint32), ("crf", C.c_int32),
                ("device_id", C.c_int32)]


_vp, _i32, _u64, _u32, _u16, _i64, _f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_uint16, C.c_int64, C.c_double
_pu64, _pmeta = C.POINTER(C.c_uint64), C.POINTER(AdderDavisMeta)
SYMBOLS = {
    "adder_davis_create": (_i32, [C.POINTER(AdderDavisParams), C.POINTER(_vp)]),
    "adder_davis_destroy": (None, [_vp]),
    "adder_davis_reset": (_i32, [_vp]),
    "adder_davis_last_error": (C.c_char_p, [_vp]),
    "adder_davis_events_per_step": (_u64, [_vp]),
    "adder_davis_push_capacity": (_u64, [_vp, _u64]),
    "adder_davis_push_device": (_i32, [_vp, _vp, _pmeta, _vp, _u64, _vp, _u64, _vp, _u64, _pu64, _pu64, _vp]),
    "adder_davis_push_host": (_i32, [_vp, _vp, _pmeta, _vp, _u64, _vp, _u64, _vp, _u64, _pu64, _pu64]),
    "adder_davis_finish_device": (_i32, [_vp, _vp, _u64, _pu64, _vp]),
    "adder_davis_finish_host": (_i32, [_vp, _vp, _u64, _pu64]),
    "adder_davis_last_frame_events": (_u64, [_vp]),
    "adder_davis_pixel_state": (_i32, [_vp, _vp, _vp]),
    "adder_davis_running_intensities": (_i32, [_vp, _vp]),
    "adder_davis_steps_host": (_i32, [_u16, _u16, _vp, _vp, _vp, _u64, _i64, _i32, _i64, _f64, _u32, _u32, _vp, _u64,
                                      _pu64, _pu64]),
    "adder_davis_gaps_host": (_i32, [_u16, _u16, _vp, _vp, _i64, _u32, _u32, _vp, _u64, _pu64]),
    "adder_davis_frame_host": (_i32, [_u16, _u16, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
}


def load():
    return N.bind(SYMBOLS)


def _events(ev):
    return np.ascontiguousarray(ev, DAVIS_EVENT_DTYPE)


def _planes(last_ts, last_ln, width, height):
    ts = np.array(last_ts, np.int64).reshape(-1)
    ln = np.array(last_ln, np.float64).reshape(-1)
    if ts.size != width * height or ln.size != width * height:
        raise ValueError("state planes of the wrong size")
    return ts, ln


def steps_host(width, height, last_ts, last_ln, events, check1, check2=None, check2_after=True, *, c, tps, ref_time,
               steps_cap=None):
    """integrate_dvs_events over one list on the CPU, by the functions the kernels run -> (steps, last_ts, last_ln):
    SPARSE_STEP_DTYPE in step order and the updated planes (copies; the arguments are left alone).  An event passes
    with t < check1 and, when check2 is given, t > check2 (check2_after) or t < check2.  A refusal raises AdderHipError
    (.index: the event outside the plane, .needed: a steps_cap that succeeds)."""
    ev = _events(events)
    ts, ln = _planes(last_ts, last_ln, width, height)
    cap = 2 * len(ev) if steps_cap is None else steps_cap
    steps = np.zeros(max(cap, 1), N.SPARSE_STEP_DTYPE)
    n, bad = C.c_uint64(0), C.c_uint64(0)
    mode2 = 0 if check2 is None else (1 if check2_after else 2)
    rc = load().adder_davis_steps_host(width, height, ts.ctypes.data, ln.ctypes.data, ev.ctypes.data if len(ev) else None,
                                       len(ev), check1, mode2, 0 if check2 is None else check2, c, tps, ref_time,
                                       steps.ctypes.data, cap, C.byref(n), C.byref(bad))
    if rc != N.OK:
        err = N.AdderHipError(rc, "adder_davis_steps_host")
        err.index = None if bad.value == NO_BAD_EVENT else bad.value
        err.needed = n.value
        err.planes = (ts.reshape(height, width), ln.reshape(height, width))
        raise err
    return steps[: n.value].copy(), ts.reshape(height, width), ln.reshape(height, width)


def gaps_host(width, height, last_ts, last_ln, start, *, tps, ref_time):
    """integrate_frame_gaps on the CPU -> (steps, last_ln): raster order; the clamp may rewrite last ln."""
    ts, ln = _planes(last_ts, last_ln, width, height)
    steps = np.zeros(width * height, N.SPARSE_STEP_DTYPE)
    n = C.c_uint64(0)
    rc = load().adder_davis_gaps_host(width, height, ts.ctypes.data, ln.ctypes.data, start, tps, ref_time,
                                      steps.ctypes.data, len(steps), C.byref(n))
    if rc != N.OK:
        raise N.AdderHipError(rc, "adder_davis_gaps_host")
    return steps[: n.value].copy(), ln.reshape(height, width)


def frame_host(width, height, mode, frame, start, end, last_ts, last_ln):
    """Steps 5 and 6 of a push on the CPU -> (image_8u, steps, last_ts, last_ln); start / end as step 1 leaves them."""
    ts, ln = _planes(last_ts, last_ln, width, height)
    f = np.ascontiguousarray(frame, np.float64).reshape(-1)
    img = np.zeros(width * height, np.uint8)
    steps = np.zeros(width * height, N.SPARSE_STEP_DTYPE)
    rc = load().adder_davis_frame_host(width, height, mode, f.ctypes.data, start, end, ts.ctypes.data, ln.ctypes.data,
                                       img.ctypes.data, steps.ctypes.data)
    if rc != N.OK:
        raise N.AdderHipError(rc, "adder_davis_frame_host: a frame value is NaN or <= -1")
    shape = (height, width)
    return img.reshape(shape), (steps if mode != FRAMED else steps[:0]), ts.reshape(shape), ln.reshape(shape)


class HipDavis(N.SourceHandle):
    """Davis::new(..)[.crf(c)] with time_parameters(tps, ref_time, delta_t_max, AbsoluteT) on one device: push() one
    packet after the other, finish() at the end of input.  After a refused push, .bad_index is the index of the event
    outside the plane (`before` first, `after` following; else None)."""
    PREFIX, DESTROY = "adder_davis", "adder_davis_destroy"

    def __init__(self, width, height, mode, tps, ref_time, delta_t_max, crf=None, device_id=0):
        self.L = load()
        p = AdderDavisParams(abi_version=ABI_VERSION, width=width, height=height, mode=mode, tps=tps, ref_time=ref_time,
                             delta_t_max=delta_t_max, crf=NO_CRF if crf is None else crf, device_id=device_id)
        h = C.c_void_p()
        rc = self.L.adder_davis_create(C.byref(p), C.byref(h))
        if rc != N.OK:
            raise N.AdderHipError(rc, (self.L.adder_davis_last_error(None) or b"").decode())
        self.h, self.params = h, p
        self.width, self.height, self.mode, self.device_id = width, height, mode, device_id
        self.events_per_step = self.L.adder_davis_events_per_step(h)
        self.bad_index = None

    def push_capacity(self, n_before):
        return self.L.adder_davis_push_capacity(self.h, n_before)

    def last_frame_events(self):
        return self.L.adder_davis_last_frame_events(self.h)

    def push(self, frame, c, start, end, before=(), after=(), has_events=True, out_cap=None, stream=None, d_out=None):
        """One packet -> its events.  frame / before / after: numpy (host form) or CUDA tensors (device form; then the
        events come back as a uint8 CUDA tensor, written into d_out when it is given).  out_cap: events of room
        (default: push_capacity), never more than d_out holds; a push that may not fit raises E_OUT_CAPACITY
        (.needed: a room that succeeds).  A refused push changes nothing."""
        self.bad_index = None
        meta = AdderDavisMeta(c=c, img_start_ts=start, img_end_ts=end, has_events=int(has_events))
        n_out, bad = C.c_uint64(0), C.c_uint64(0)
        if isinstance(frame, np.ndarray) or frame is None:
            f = None if frame is None else np.ascontiguousarray(frame, np.float64)
            if f is not None and f.size != self.width * self.height:
                raise ValueError("a frame of the wrong size")
            b, a = _events(before), _events(after)
            if out_cap is None:
                out_cap = self.push_capacity(len(b))
            out = np.zeros(max(out_cap, 1), N.EVENT_DTYPE)
            rc = self.L.adder_davis_push_host(self.h, None if f is None else f.ctypes.data, C.byref(meta),
                                              b.ctypes.data if len(b) else None, len(b),
                                              a.ctypes.data if len(a) else None, len(a), out.ctypes.data, out_cap,
                                              C.byref(n_out), C.byref(bad))
            self._done(rc, bad, n_out)
            return out[: n_out.value].copy()
        import torch
        dev = torch.device(f"cuda:{self.device_id}")
        N.device_buffer(frame, dev, "frame")
        if frame.dtype != torch.float64 or frame.numel() != self.width * self.height:
            raise ValueError("frame: float64, width * height values")

        def lst(t, what):
            if t is None or (not hasattr(t, "is_cuda") and len(t) == 0):
                return None, 0
            N.device_buffer(t, dev, what)
            n = t.numel() * t.element_size() // 16
            return (t.data_ptr() if n else None), n
        pb, nb = lst(before, "before")
        pa, na = lst(after, "after")
        if out_cap is None:
            out_cap = self.push_capacity(nb)
        d_out, out_cap = self._device_out(dev, out_cap, d_out)
        rc = self.L.adder_davis_push_device(self.h, frame.data_ptr(), C.byref(meta), pb, nb, pa, na, d_out.data_ptr(),
                                            out_cap, C.byref(n_out), C.byref(bad), C.c_void_p(stream) if stream else None)
        self._done(rc, bad, n_out)
        return d_out[: n_out.value * 12]

    def pixel_state(self):
        """The camera state the last accepted push left -> (last ts, last ln): (H, W) int64 and float64 planes."""
        ts = np.zeros((self.height, self.width), np.int64)
        ln = np.zeros((self.height, self.width), np.float64)
        self._check(self.L.adder_davis_pixel_state(self.h, ts.ctypes.data, ln.ctypes.data))
        return ts, ln


def davis_to_adder(packets, width, height, mode, *, tps, ref_time, delta_t_max, crf=None, device_id=0, sink=None):
    """Every event the Davis source feeds its encoder for these packets (dicts {frame, c, start, end, before, after}),
    the final flush included, in order.  With `sink` the events of each push go to sink(events) instead of being
    collected, and the number of events is returned."""
    dv = HipDavis(width, height, mode, tps, ref_time, delta_t_max, crf, device_id)
    out, n = [], 0
    try:
        for pk in packets:
            ev = dv.push(np.asarray(pk["frame"], np.float64), float(pk["c"]), int(pk["start"]), int(pk["end"]),
                         pk.get("before", ()), pk.get("after", ()), has_events=mode != FRAMED)
            n += len(ev)
            sink(ev) if sink else out.append(ev)
        ev = dv.finish()
        n += len(ev)
        sink(ev) if sink else out.append(ev)
    finally:
        dv.close()
    if sink:
        return n
    return np.concatenate(out) if out else np.zeros(0, N.EVENT_DTYPE)


def davis_to_adder_file(packets, out, width, height, mode, *, tps, ref_time, delta_t_max, crf=None, device_id=0):
    """The packets as a raw .adder file: header (DavisU8, AbsoluteT), every event in the source's order, the EOF event.
    -> dict(width, height, packets, events)."""
    from .video import raw_header, raw_events, raw_eof
    packets = list(packets)
    with open(out, "wb") as g:
        g.write(raw_header(CODEC_VERSION, width, height, 1, tps, ref_time, delta_t_max,
                           source_camera=SOURCE_CAMERA_DAVIS_U8, time_mode=N.TIME_ABSOLUTE_T))
        n = davis_to_adder(packets, width, height, mode, tps=tps, ref_time=ref_time, delta_t_max=delta_t_max, crf=crf,
                           device_id=device_id, sink=lambda ev: g.write(raw_events(ev, 1)))
        g.write(raw_eof())
    return dict(width=width, height=height, packets=len(packets), events=n)
