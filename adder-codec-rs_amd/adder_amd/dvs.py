"""HipDvs: ctypes binding of the ADDER -> DVS conversion in libadder_hip.so (include/adder_dvs.h), and
adder_to_dvs_file, the reference's adder-to-dvs tool (a raw .adder file -> Prophesee .dat or text) streamed through
the device batch by batch.

Inputs are numpy arrays (host forms of the C-ABI) or torch device tensors (device forms): AdderEvents (EVENT_DTYPE,
or their bytes) or the 9 / 11-byte wire records of a .adder body.  Outputs are DVS_EVENT_DTYPE (the full time) or
DAT_DTYPE (the .dat record).

HipDvs.enable_video turns on the tool's other half: the DVS event video ([h][w] gray planes, 255 on / 0 off / 128
blank, with their frame indices) and the per-unit event-count map.
"""
import ctypes as C
import datetime

import numpy as np

from . import _native as N

ABI_VERSION = 1
OUT_EVENTS, OUT_DAT = 0, 1
E_BAD_EVENT = -16
NO_BAD_EVENT = (1 << 64) - 1

DVS_EVENT_DTYPE = np.dtype([("t", "<u8"), ("x", "<u2"), ("y", "<u2"), ("p", "u1"), ("pad", "u1", (3,))])
DAT_DTYPE = np.dtype([("t", "<u4"), ("w", "<u4")])  # w = p << 28 | y << 14 | x
assert DVS_EVENT_DTYPE.itemsize == 16 and DAT_DTYPE.itemsize == 8


class AdderDvsParams(C.Structure):
    """include/adder_dvs.h::AdderDvsParams"""
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("width", C.c_uint16),
        ("height", C.c_uint16),
        ("channels", C.c_uint8),
        ("time_mode", C.c_uint8),
        ("reserved0", C.c_uint16),
        ("ref_interval", C.c_uint32),
        ("source_camera", C.c_uint32),
        ("theta", C.c_double),
        ("device_id", C.c_int32),
    ]


class AdderDvsVideoParams(C.Structure):
    """include/adder_dvs.h::AdderDvsVideoParams"""
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("tps", C.c_uint32),
        ("fps", C.c_float),
        ("buffer_secs", C.c_float),
        ("ring_frames", C.c_uint32),
        ("draw", C.c_uint32),
    ]


_vp, _i32, _u64, _sz = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t
_pu64, _pu32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
SYMBOLS = {
    "adder_dvs_parse_header": (_i32, [_vp, _sz, C.POINTER(AdderDvsParams), _pu32, _pu32]),
    "adder_dvs_create": (_i32, [C.POINTER(AdderDvsParams), C.POINTER(_vp)]),
    "adder_dvs_destroy": (None, [_vp]),
    "adder_dvs_reset": (_i32, [_vp]),
    "adder_dvs_last_error": (C.c_char_p, [_vp]),
    "adder_dvs_convert_device": (_i32, [_vp, _vp, _u64, _i32, _vp, _u64, _pu64, _pu64, _vp]),
    "adder_dvs_convert_wire_device": (_i32, [_vp, _vp, _u64, _i32, _vp, _u64, _pu64, _pu64, _pu64, _vp]),
    "adder_dvs_convert_host": (_i32, [_vp, _vp, _u64, _i32, _vp, _u64, _pu64, _pu64]),
    "adder_dvs_convert_wire_host": (_i32, [_vp, _vp, _u64, _i32, _vp, _u64, _pu64, _pu64, _pu64]),
    "adder_dvs_sort_device": (_i32, [_vp, _vp, _u64, _i32, _vp]),
    "adder_dvs_header_bytes": (_sz, [C.c_uint16, C.c_uint16, C.c_char_p, _i32, _vp, _sz]),
    "adder_dvs_format_text": (_sz, [_vp, _u64, _vp, _sz]),
    "adder_dvs_log1p": (C.c_double, [C.c_double]),
    "adder_dvs_log1p_host": (None, [_vp, _vp, _u64]),
    "adder_dvs_log1p_device": (_i32, [_vp, _vp, _u64, _i32]),
    "adder_dvs_video_params_from_header": (_i32, [_vp, _sz, C.POINTER(AdderDvsVideoParams)]),
    "adder_dvs_video_enable": (_i32, [_vp, C.POINTER(AdderDvsVideoParams)]),
    "adder_dvs_video_frames_ready": (_i32, [_vp, _pu64]),
    "adder_dvs_video_ring_needed": (_i32, [_vp, _pu64]),
    "adder_dvs_video_pop_device": (_i32, [_vp, _vp, _u64, _vp, _pu64, _vp]),
    "adder_dvs_video_pop": (_i32, [_vp, _vp, _u64, _vp, _pu64]),
    "adder_dvs_video_finish": (_i32, [_vp]),
    "adder_dvs_event_count_map_device": (_i32, [_vp, _vp, _vp]),
    "adder_dvs_event_count_map": (_i32, [_vp, _vp]),
    "adder_dvs_video_params_check": (_i32, [C.POINTER(AdderDvsVideoParams), _pu64, _pu64]),
    "adder_dvs_video_frame_length": (_u64, [C.c_uint32, C.c_float]),
    "adder_dvs_video_buffer_ticks": (_u64, [C.c_uint32, C.c_float]),
    "adder_dvs_video_count_byte": (C.c_uint8, [C.c_uint32, C.c_uint32]),
    "adder_dvs_video_schedule_host": (_u64, [_vp, _vp, _u64, _u64, _u64, _i32, _vp, _vp, _vp, _vp, _u64]),
}


def load():
    return N.bind(SYMBOLS)


def log1p(x):
    """The library's binary64 log1p on the host (the routine the kernels evaluate): a float, or a float64 array."""
    if np.ndim(x) == 0:
        return load().adder_dvs_log1p(float(x))
    xs = np.ascontiguousarray(x, dtype=np.float64)
    ys = np.empty_like(xs)
    load().adder_dvs_log1p_host(xs.ctypes.data, ys.ctypes.data, xs.size)
    return ys


def log1p_device(x, device_id=0):
    """The same routine evaluated by a kernel (self-test): float64 array in, float64 array out."""
    import torch
    dev = f"cuda:{device_id}"
    xs = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    ys = torch.empty_like(xs)
    rc = load().adder_dvs_log1p_device(xs.data_ptr(), ys.data_ptr(), xs.numel(), device_id)
    if rc != N.OK:
        raise N.AdderHipError(rc, "device log1p")
    return ys.cpu().numpy()


def parse_header(buf):
    """-> (meta dict: width, height, channels, time_mode, ref_interval, source_camera; header bytes; event bytes)."""
    b = bytes(buf[:64])
    p, hb, eb = AdderDvsParams(), C.c_uint32(0), C.c_uint32(0)
    rc = load().adder_dvs_parse_header(b, len(b), C.byref(p), C.byref(hb), C.byref(eb))
    if rc != N.OK:
        raise N.AdderHipError(rc, "not a raw .adder header of codec version 0..3")
    meta = dict(width=p.width, height=p.height, channels=p.channels, time_mode=p.time_mode,
                ref_interval=p.ref_interval, source_camera=p.source_camera)
    return meta, hb.value, eb.value


def video_params_from_header(buf):
    """-> AdderDvsVideoParams with the header's tps and the CLI's defaults (fps 100, buffer_secs 10, draw)."""
    b = bytes(buf[:64])
    p = AdderDvsVideoParams()
    rc = load().adder_dvs_video_params_from_header(b, len(b), C.byref(p))
    if rc != N.OK:
        raise N.AdderHipError(rc, "not a raw .adder header of codec version 0..3")
    return p


def video_params_check(tps, fps=100.0, buffer_secs=10.0, draw=True, ring_frames=0, abi_version=ABI_VERSION):
    """What enable_video asks of its parameters, without a device -> (code, L, B): frame length and buffer in ticks."""
    p = AdderDvsVideoParams(abi_version=abi_version, tps=tps, fps=fps, buffer_secs=buffer_secs,
                            ring_frames=ring_frames, draw=1 if draw else 0)
    fl, b = C.c_uint64(0), C.c_uint64(0)
    rc = load().adder_dvs_video_params_check(C.byref(p), C.byref(fl), C.byref(b))
    return rc, fl.value, b.value


def video_schedule_host(pt, fire_t, L, B, state=(0, 0, 1), draw=True):
    """The library's video schedule of one call on the host (the arithmetic the kernels run): per event the unit's
    time after it (0: a first event) and old_t + 1 of a fired event (0: none); state = (frame_count, current_t, end)
    -> (pop marks, accept marks, emitted frame indices, state after)."""
    pt = np.ascontiguousarray(pt, dtype=np.uint64)
    ft = np.ascontiguousarray(fire_t, dtype=np.uint64)
    n = len(pt)
    pop, acc, em = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    st = np.array(state, np.uint64)
    k = load().adder_dvs_video_schedule_host(pt.ctypes.data if n else None, ft.ctypes.data if n else None, n, L, B,
                                             1 if draw else 0, st.ctypes.data, pop.ctypes.data if n else None,
                                             acc.ctypes.data if n else None, em.ctypes.data if n else None, n)
    return pop, acc, em[:k], tuple(int(v) for v in st)


def header_bytes(width, height, date, binary=True):
    """The .dat / text header (main.rs:151-163); `date` is the caller's "YYYY-mm-dd HH:MM:SS"."""
    L = load()
    d = date.encode()
    n = L.adder_dvs_header_bytes(width, height, d, 1 if binary else 0, None, 0)
    buf = C.create_string_buffer(n)
    L.adder_dvs_header_bytes(width, height, d, 1 if binary else 0, buf, n)
    return buf.raw[:n]


def format_text(events):
    """DVS_EVENT_DTYPE records -> b"t x y p\\n" lines (main.rs:486-498)."""
    ev = np.ascontiguousarray(events, dtype=DVS_EVENT_DTYPE)
    L = load()
    n = L.adder_dvs_format_text(ev.ctypes.data, len(ev), None, 0)
    buf = C.create_string_buffer(max(n, 1))
    L.adder_dvs_format_text(ev.ctypes.data, len(ev), buf, n)
    return buf.raw[:n]


class HipDvs(N.Handle):
    """Per-unit DVS state on one device.  Every convert call continues the stream where the last one stopped.

    After a call: .bad_index is the index (within that call's input) of the event that stopped it, or None -- the
    events before it are applied and their output returned, nothing after it is; .consumed is the number of wire
    records before an EOF record (all of them when there is none)."""
    DESTROY = "adder_dvs_destroy"

    def __init__(self, width, height, channels=1, time_mode=N.TIME_DELTA_T, ref_interval=255, source_camera=0,
                 theta=0.01, device_id=0):
        self.L = load()
        p = AdderDvsParams(abi_version=ABI_VERSION, width=width, height=height, channels=channels,
                           time_mode=time_mode, ref_interval=ref_interval, source_camera=source_camera,
                           theta=float(theta), device_id=device_id)
        h = C.c_void_p()
        rc = self.L.adder_dvs_create(C.byref(p), C.byref(h))
        if rc != N.OK:
            raise N.AdderHipError(rc, (self.L.adder_dvs_last_error(None) or b"").decode())
        self.h, self.params = h, p
        self.record_bytes = 9 if channels == 1 else 11
        self.bad_index, self.consumed = None, 0
        self.ring_needed = 0
        self._video = False

    def enable_video(self, tps, fps=100.0, buffer_secs=10.0, draw=True, ring_frames=0):
        """Turns on the event video and the count map (before the first event, or after a reset).  ring_frames 0:
        ceil(B / L) + 64 planes on the device.  A convert call that needs more raises AdderHipError(E_OUT_CAPACITY)
        and changes nothing; .ring_needed then holds the slots it asked for."""
        p = AdderDvsVideoParams(abi_version=ABI_VERSION, tps=tps, fps=fps, buffer_secs=buffer_secs,
                                ring_frames=ring_frames, draw=1 if draw else 0)
        self._check(self.L.adder_dvs_video_enable(self.h, C.byref(p)))
        self._video = True

    def video_ready(self):
        n = C.c_uint64(0)
        self._check(self.L.adder_dvs_video_frames_ready(self.h, C.byref(n)))
        return n.value

    def video_ring_needed(self):
        """ring slots the last convert or finish call needed"""
        n = C.c_uint64(0)
        self._check(self.L.adder_dvs_video_ring_needed(self.h, C.byref(n)))
        return n.value

    def video_pop(self, device=False, rgb=False, stream=None):
        """The frames emitted since the last pop -> (frame indices: uint64 array, [n][h][w] uint8 planes: numpy, or a
        CUDA tensor with device=True).  rgb: [n][h][w][3], the plane three times (the reference's frame)."""
        n = self.video_ready()
        w, h = self.params.width, self.params.height
        idx, got = np.zeros(max(n, 1), np.uint64), C.c_uint64(0)
        if device:
            import torch
            out = torch.empty((max(n, 1), h, w), dtype=torch.uint8, device=f"cuda:{self.params.device_id}")
            self._check(self.L.adder_dvs_video_pop_device(self.h, out.data_ptr(), n, idx.ctypes.data, C.byref(got),
                                                          C.c_void_p(stream) if stream else None))
            out = out[: got.value]
            return idx[: got.value], (out[..., None].expand(-1, -1, -1, 3).contiguous() if rgb else out)
        out = np.zeros((max(n, 1), h, w), np.uint8)
        self._check(self.L.adder_dvs_video_pop(self.h, out.ctypes.data, n, idx.ctypes.data, C.byref(got)))
        out = out[: got.value]
        return idx[: got.value], (np.repeat(out[..., None], 3, axis=-1) if rgb else out)

    def video_finish(self):
        """The stream's end: the final check; every pending frame (or one blank frame) becomes ready to pop."""
        self._check(self.L.adder_dvs_video_finish(self.h))

    def event_count_map(self, device=False, stream=None):
        """-> [h][w][3] uint8 (numpy, or a CUDA tensor with device=True)."""
        w, h = self.params.width, self.params.height
        if device:
            import torch
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=f"cuda:{self.params.device_id}")
            self._check(self.L.adder_dvs_event_count_map_device(self.h, out.data_ptr(),
                                                                C.c_void_p(stream) if stream else None))
            return out
        out = np.zeros((h, w, 3), np.uint8)
        self._check(self.L.adder_dvs_event_count_map(self.h, out.ctypes.data))
        return out

    @classmethod
    def from_header(cls, buf, theta=0.01, device_id=0):
        meta, _, _ = parse_header(buf)
        return cls(theta=theta, device_id=device_id, **meta)

    def reset(self):
        self._check(self.L.adder_dvs_reset(self.h))

    def _check(self, rc):
        if rc not in (N.OK, E_BAD_EVENT):
            msg = (self.L.adder_dvs_last_error(self.h) or b"").decode()
            need = C.c_uint64(0)
            if rc == N.E_OUT_CAPACITY and self._video and \
                    self.L.adder_dvs_video_ring_needed(self.h, C.byref(need)) == N.OK:
                self.ring_needed = need.value
            raise N.AdderHipError(rc, msg)

    def _done(self, rc, bad, consumed):
        self._check(rc)
        self.bad_index = None if bad.value == NO_BAD_EVENT else bad.value
        self.consumed = consumed

    def convert(self, events, out_format=OUT_EVENTS, stream=None):
        """AdderEvents: a numpy EVENT_DTYPE array (host form) or a torch CUDA tensor of their bytes (device form).
        -> the fired DVS records (numpy array / uint8 CUDA tensor of whole records)."""
        if isinstance(events, np.ndarray):
            ev = np.ascontiguousarray(events, dtype=N.EVENT_DTYPE)
            return self._host(self.L.adder_dvs_convert_host, ev, len(ev), out_format, wire=False)
        n = events.numel() * events.element_size() // 12
        return self._device(self.L.adder_dvs_convert_device, events, n, out_format, stream, wire=False)

    def convert_wire(self, records, out_format=OUT_EVENTS, stream=None):
        """Wire records (the body of a .adder file): numpy uint8 / bytes (host form) or a uint8 CUDA tensor."""
        rb = self.record_bytes
        if isinstance(records, (bytes, bytearray, memoryview, np.ndarray)):
            w = np.frombuffer(records, np.uint8) if not isinstance(records, np.ndarray) else \
                np.ascontiguousarray(records).view(np.uint8).reshape(-1)
            return self._host(self.L.adder_dvs_convert_wire_host, w, w.size // rb, out_format, wire=True)
        n = records.numel() * records.element_size() // rb
        return self._device(self.L.adder_dvs_convert_wire_device, records, n, out_format, stream, wire=True)

    def _host(self, fn, arr, n, out_format, wire):
        dt = DAT_DTYPE if out_format == OUT_DAT else DVS_EVENT_DTYPE
        out = np.zeros(max(n, 1), dt)
        n_out, bad, consumed = C.c_uint64(0), C.c_uint64(0), C.c_uint64(n)
        args = [self.h, arr.ctypes.data if n else None, n, out_format, out.ctypes.data, n, C.byref(n_out),
                C.byref(bad)]
        if wire:
            args.append(C.byref(consumed))
        self._done(fn(*args), bad, consumed.value)
        return out[: n_out.value]

    def _device(self, fn, t, n, out_format, stream, wire):
        import torch
        rb = 8 if out_format == OUT_DAT else 16
        out = torch.empty(max(n, 1) * rb, dtype=torch.uint8, device=t.device)
        n_out, bad, consumed = C.c_uint64(0), C.c_uint64(0), C.c_uint64(n)
        args = [self.h, t.data_ptr() if n else None, n, out_format, out.data_ptr(), n, C.byref(n_out), C.byref(bad)]
        if wire:
            args.append(C.byref(consumed))
        args.append(C.c_void_p(stream) if stream else None)
        self._done(fn(*args), bad, consumed.value)
        return out[: n_out.value * rb]

    def sort(self, records, out_format=OUT_DAT, stream=None):
        """--reorder: stable sort by the 32-bit time, in place, of a uint8 CUDA tensor of records (device form) or a
        numpy record array (copied to the device and back; returned)."""
        if isinstance(records, np.ndarray):
            import torch
            d = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1).copy()).to(
                f"cuda:{self.params.device_id}")
            self.sort(d, out_format)
            return np.frombuffer(d.cpu().numpy().tobytes(), records.dtype)
        rb = 8 if out_format == OUT_DAT else 16
        self._check(self.L.adder_dvs_sort_device(self.h, records.data_ptr(), records.numel() // rb, out_format,
                                                 C.c_void_p(stream) if stream else None))
        return records


def adder_to_dvs_file(in_path, out_path, *, text=False, theta=0.01, reorder=False, date=None,
                      batch_records=1 << 24, device_id=0, video_path=None, fps=100.0, buffer_secs=10.0, draw=True,
                      counts_path=None, playback_slowdown=1.0, ring_frames=0):
    """adder-to-dvs: a raw .adder file -> DVS events, Prophesee .dat (binary) or "t x y p" lines (text=True).
    The file is streamed through the device in batches of batch_records wire records.  reorder (binary only):
    the whole output is kept on the device and written after a stable sort by 32-bit t.  date: the header's
    "YYYY-mm-dd HH:MM:SS" (default: now).  A bad event (see include/adder_dvs.h) ends the run like the reference's:
    the output before it is written (with reorder: none of it) and AdderHipError(E_BAD_EVENT) is raised, its
    .index the event's index in the file.

    video_path: the DVS event video (fps, buffer_secs, draw as the reference's CLI) as raw [n][h][w] gray8 planes,
    and video_path + ".times" with one line per written frame, the time the reference stamps it with
    (k-th frame: k / fps / playback_slowdown, accumulated as it does).  counts_path: the event-count map,
    [h][w][3] bytes.  Neither is written past a bad event's batch.  A batch that asks for more ring frames than there
    are is converted in smaller pieces.  -> dict(events_in, events_out[, frames])."""
    if date is None:
        date = datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")
    reorder = reorder and not text  # the queue is only fed in binary mode (main.rs:501-524)
    fmt = OUT_EVENTS if text else OUT_DAT
    video = video_path is not None or counts_path is not None
    vf = open(video_path, "wb") if video_path is not None else None
    times = []

    def drain(dvs):
        _, planes = dvs.video_pop()
        for _ in range(len(planes)):  # current_frame_time += 1.0 / fps as f64 after every written frame
            times.append(times[-1] + 1.0 / float(np.float32(fps)) if times else 0.0)
        if vf is not None:
            vf.write(planes.tobytes())

    dvs = None
    try:  # whatever ends the run, the video file is closed and the frames written so far keep their times
        with open(in_path, "rb") as f:
            head = f.read(64)
            meta, hb, eb = parse_header(head)
            f.seek(hb)
            dvs = HipDvs(theta=theta, device_id=device_id, **meta)
            if video:
                dvs.enable_video(video_params_from_header(head).tps, fps, buffer_secs, draw, ring_frames)
            n_in = n_out = 0
            kept = []
            bad = None
            with open(out_path, "wb") as g:
                g.write(header_bytes(meta["width"], meta["height"], date, binary=not text))
                done = False
                while not done:
                    buf = f.read(batch_records * eb)
                    n = len(buf) // eb
                    if n == 0:
                        break
                    pos, size = 0, n
                    while pos < n and not done:
                        m = min(size, n - pos)
                        piece = buf[pos * eb: (pos + m) * eb]
                        try:
                            if reorder:
                                import torch
                                d = torch.frombuffer(bytearray(piece), dtype=torch.uint8).to(f"cuda:{device_id}")
                                recs = dvs.convert_wire(d, fmt)
                            else:
                                recs = dvs.convert_wire(piece, fmt)
                        except N.AdderHipError as e:
                            if not video or e.code != N.E_OUT_CAPACITY or m < 2:
                                raise
                            size = m // 2  # nothing was changed: the same events again, fewer at a time
                            continue
                        if reorder:
                            kept.append(recs)
                        else:
                            g.write(format_text(recs) if text else recs.tobytes())
                        if video:
                            drain(dvs)
                        n_in += dvs.consumed if dvs.bad_index is None else dvs.bad_index
                        n_out += len(recs) if not reorder else recs.numel() // 8
                        if dvs.bad_index is not None:
                            bad = n_in
                            done = True
                        elif dvs.consumed < m:
                            done = True
                        pos += m
                    if n < batch_records:
                        done = True
                if reorder and bad is None and n_out:
                    import torch
                    allr = torch.cat(kept)
                    dvs.sort(allr, OUT_DAT)
                    g.write(allr.cpu().numpy().tobytes())
            if video and bad is None:
                dvs.video_finish()
                drain(dvs)
                if counts_path is not None:
                    with open(counts_path, "wb") as c:
                        c.write(dvs.event_count_map().tobytes())
    finally:
        if dvs is not None:
            dvs.close()
        if vf is not None:
            vf.close()
            with open(video_path + ".times", "wb") as tf:
                tf.write("".join("%.9f\n" % (t / playback_slowdown) for t in times).encode())
    if bad is not None:
        err = N.AdderHipError(E_BAD_EVENT, f"event {bad} of {in_path} cannot be converted to DVS")
        err.index = bad
        raise err
    res = dict(events_in=n_in, events_out=n_out)
    if video:
        res["frames"] = len(times)
    return res
