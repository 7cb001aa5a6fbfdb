"""HipPlayer: ctypes binding of the latest-event video player in libadder_hip.so (include/adder_player.h), and
play_file, the reference's adder_video_player (a raw .adder file -> the frames it would show) streamed through the
device batch by batch.

Inputs are numpy arrays (host forms of the C-ABI) or torch device tensors (device forms): AdderEvents (EVENT_DTYPE,
or their bytes) or the 9 / 11-byte wire records of a .adder body.  Frames are [n][height][width][channels] arrays of
float64 (the reference's matrix) or uint8 (saturate(rint(v * 255)), ours).
"""
import ctypes as C

import numpy as np

from . import _native as N

ABI_VERSION = 1
F64, U8 = 0, 1
E_BAD_EVENT = -16
NO_BAD_EVENT = (1 << 64) - 1
OUT_TYPES = {"f64": F64, "u8": U8}


class AdderPlayerParams(C.Structure):
    """include/adder_player.h::AdderPlayerParams"""
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("width", C.c_uint16),
        ("height", C.c_uint16),
        ("channels", C.c_uint8),
        ("time_mode", C.c_uint8),
        ("reserved0", C.c_uint16),
        ("ref_interval", C.c_uint32),
        ("tps", C.c_uint32),
        ("source_camera", C.c_uint32),
        ("playback_fps", C.c_double),
        ("out_type", C.c_int32),
        ("device_id", C.c_int32),
    ]


_vp, _i32, _u64, _sz = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t
_pu64, _pu32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
SYMBOLS = {
    "adder_player_parse_header": (_i32, [_vp, _sz, C.POINTER(AdderPlayerParams), _pu32, _pu32]),
    "adder_player_create": (_i32, [C.POINTER(AdderPlayerParams), C.POINTER(_vp)]),
    "adder_player_destroy": (None, [_vp]),
    "adder_player_reset": (_i32, [_vp]),
    "adder_player_last_error": (C.c_char_p, [_vp]),
    "adder_player_play_device": (_i32, [_vp, _vp, _u64, _vp, _u64, _pu64, _pu64, _vp]),
    "adder_player_play_wire_device": (_i32, [_vp, _vp, _u64, _vp, _u64, _pu64, _pu64, _pu64, _vp]),
    "adder_player_finish": (_i32, [_vp, _vp, _u64, _pu64, _vp]),
    "adder_player_play_host": (_i32, [_vp, _vp, _u64, _vp, _u64, _pu64, _pu64]),
    "adder_player_play_wire_host": (_i32, [_vp, _vp, _u64, _vp, _u64, _pu64, _pu64, _pu64]),
    "adder_player_display_device": (_i32, [_vp, _vp, _vp]),
    "adder_player_display": (_i32, [_vp, _vp]),
    "adder_player_clock": (_i32, [_vp, _pu32, _pu64]),
    "adder_player_schedule_host": (None, [_vp, _u64, _u64, _u64, _vp]),
    "adder_player_frame_length": (_u64, [C.c_uint32, C.c_double]),
}


def load():
    return N.bind(SYMBOLS)


def parse_header(buf):
    """-> (meta dict: width, height, channels, time_mode, ref_interval, tps, source_camera; header bytes; event
    bytes)."""
    b = bytes(buf[:64])
    p, hb, eb = AdderPlayerParams(), C.c_uint32(0), C.c_uint32(0)
    rc = load().adder_player_parse_header(b, len(b), C.byref(p), C.byref(hb), C.byref(eb))
    if rc != N.OK:
        raise N.AdderHipError(rc, "not a raw .adder header of codec version 0..3")
    meta = dict(width=p.width, height=p.height, channels=p.channels, time_mode=p.time_mode,
                ref_interval=p.ref_interval, tps=p.tps, source_camera=p.source_camera)
    return meta, hb.value, eb.value


def frame_length(tps, playback_fps):
    """(tps as f64 / playback_fps) as an integer, clamped to 2^32: the library's FL."""
    return load().adder_player_frame_length(tps, float(playback_fps))


def schedule_host(cur_before, f0, fl):
    """The library's display schedule on the host (the prefix-minimum form the kernels use): current_t before each
    check, the carried frame_count and the frame length -> uint8 marks."""
    cur = np.ascontiguousarray(cur_before, dtype=np.uint32)
    marks = np.zeros(len(cur), np.uint8)
    load().adder_player_schedule_host(cur.ctypes.data if len(cur) else None, len(cur), f0, fl,
                                      marks.ctypes.data if len(cur) else None)
    return marks


class HipPlayer(N.Handle):
    """The player's state on one device.  Every play call continues the stream where the last one stopped.

    After a call: .bad_index is the index (within that call's input) of the event that stopped it, or None -- the
    events before it are applied and their frames returned, nothing after it is; .consumed is the number of wire
    records before an EOF record (all of them when there is none).

    A call whose frames do not fit max_frames raises AdderHipError(E_OUT_CAPACITY) with .needed = the count, and
    changes nothing."""
    DESTROY = "adder_player_destroy"

    def __init__(self, width, height, channels=1, time_mode=N.TIME_DELTA_T, ref_interval=255, tps=255 * 30,
                 source_camera=0, playback_fps=60.0, out="f64", device_id=0):
        self.L = load()
        p = AdderPlayerParams(abi_version=ABI_VERSION, width=width, height=height, channels=channels,
                              time_mode=time_mode, ref_interval=ref_interval, tps=tps, source_camera=source_camera,
                              playback_fps=float(playback_fps), out_type=OUT_TYPES.get(out, out), device_id=device_id)
        h = C.c_void_p()
        rc = self.L.adder_player_create(C.byref(p), C.byref(h))
        if rc != N.OK:
            raise N.AdderHipError(rc, (self.L.adder_player_last_error(None) or b"").decode())
        self.h, self.params = h, p
        self.record_bytes = 9 if channels == 1 else 11
        self.shape = (height, width, channels)
        self.units = height * width * channels
        self.dtype = np.dtype(np.uint8 if p.out_type == U8 else np.float64)
        self.bad_index, self.consumed = None, 0

    @classmethod
    def from_header(cls, buf, playback_fps=60.0, out="f64", device_id=0):
        meta, _, _ = parse_header(buf)
        return cls(playback_fps=playback_fps, out=out, device_id=device_id, **meta)

    def reset(self):
        self._check(self.L.adder_player_reset(self.h), 0)

    def clock(self):
        """-> (current_t, frame_count)"""
        t, f = C.c_uint32(0), C.c_uint64(0)
        self._check(self.L.adder_player_clock(self.h, C.byref(t), C.byref(f)), 0)
        return t.value, f.value

    def _check(self, rc, needed):
        if rc not in (N.OK, E_BAD_EVENT):
            err = N.AdderHipError(rc, (self.L.adder_player_last_error(self.h) or b"").decode())
            err.needed = needed
            raise err

    def _done(self, rc, n_frames, bad, consumed):
        self._check(rc, n_frames.value)
        self.bad_index = None if bad.value == NO_BAD_EVENT else bad.value
        self.consumed = consumed

    def play(self, events, max_frames=None, stream=None, frames=None):
        """AdderEvents: a numpy EVENT_DTYPE array (host form) or a torch CUDA tensor of their bytes (device form).
        -> the frames this batch shows (numpy array / CUDA tensor), [n, height, width, channels].  max_frames: the
        room to offer (default: one frame per record, which always fits).  frames (device form): a CUDA tensor of
        the player's dtype to write into; its whole frames are the room."""
        if isinstance(events, np.ndarray):
            ev = np.ascontiguousarray(events, dtype=N.EVENT_DTYPE)
            return self._host(self.L.adder_player_play_host, ev, len(ev), max_frames, wire=False)
        n = events.numel() * events.element_size() // 12
        return self._device(self.L.adder_player_play_device, events, n, max_frames, stream, False, frames)

    def play_wire(self, records, max_frames=None, stream=None, frames=None):
        """Wire records (the body of a .adder file): numpy uint8 / bytes (host form) or a uint8 CUDA tensor."""
        rb = self.record_bytes
        if isinstance(records, (bytes, bytearray, memoryview, np.ndarray)):
            w = np.frombuffer(records, np.uint8) if not isinstance(records, np.ndarray) else \
                np.ascontiguousarray(records).view(np.uint8).reshape(-1)
            return self._host(self.L.adder_player_play_wire_host, w, w.size // rb, max_frames, wire=True)
        n = records.numel() * records.element_size() // rb
        return self._device(self.L.adder_player_play_wire_device, records, n, max_frames, stream, True, frames)

    def finish(self, stream=None):
        """The stream's last check for the AdderEvent form (play_wire makes it at the EOF record): 0 or 1 frames,
        a CUDA tensor."""
        import torch
        out = torch.empty((1,) + self.shape, dtype=getattr(torch, self.dtype.name),
                          device=f"cuda:{self.params.device_id}")
        n_frames = C.c_uint64(0)
        rc = self.L.adder_player_finish(self.h, out.data_ptr(), 1, C.byref(n_frames),
                                        C.c_void_p(stream) if stream else None)
        self._check(rc, n_frames.value)
        return out[: n_frames.value]

    def _room(self, n, max_frames):
        """-> (the most frames the caller accepts, the room of the first attempt: what fits in 64 MB)"""
        cap = n + 1 if max_frames is None else max_frames
        return cap, min(cap, max(1, (64 << 20) // (self.units * self.dtype.itemsize)))

    def _host(self, fn, arr, n, max_frames, wire):
        cap, room = self._room(n, max_frames)
        n_frames, bad, consumed = C.c_uint64(0), C.c_uint64(NO_BAD_EVENT), C.c_uint64(n)
        out = np.empty((room,) + self.shape, self.dtype)
        args = [self.h, arr.ctypes.data if n else None, n, out.ctypes.data, room, C.byref(n_frames), C.byref(bad)]
        if wire:
            args.append(C.byref(consumed))
        rc = fn(*args)
        if rc == N.E_OUT_CAPACITY and n_frames.value <= cap:  # nothing changed: again, with the room it asks for
            out = np.empty((n_frames.value,) + self.shape, self.dtype)
            args[3], args[4] = out.ctypes.data, n_frames.value
            rc = fn(*args)
        self._done(rc, n_frames, bad, consumed.value)
        return out[: n_frames.value]

    def _device(self, fn, t, n, max_frames, stream, wire, frames=None):
        import torch
        cap, room = self._room(n, max_frames)
        if frames is not None:
            cap = room = frames.numel() // self.units
        n_frames, bad, consumed = C.c_uint64(0), C.c_uint64(NO_BAD_EVENT), C.c_uint64(n)
        mk = lambda k: torch.empty((k,) + self.shape, dtype=getattr(torch, self.dtype.name), device=t.device)
        out = mk(room) if frames is None else frames.reshape(-1)[: room * self.units].reshape((room,) + self.shape)
        args = [self.h, t.data_ptr() if n else None, n, out.data_ptr(), room, C.byref(n_frames), C.byref(bad)]
        if wire:
            args.append(C.byref(consumed))
        args.append(C.c_void_p(stream) if stream else None)
        rc = fn(*args)
        if rc == N.E_OUT_CAPACITY and n_frames.value <= cap and frames is None:
            out = mk(n_frames.value)
            args[3], args[4] = out.data_ptr(), n_frames.value
            rc = fn(*args)
        self._done(rc, n_frames, bad, consumed.value)
        return out[: n_frames.value]

    def display(self, device=False):
        """The matrix as it stands now, without a check: [height, width, channels], numpy (or a CUDA tensor)."""
        if device:
            import torch
            out = torch.empty(self.shape, dtype=getattr(torch, self.dtype.name), device=f"cuda:{self.params.device_id}")
            self._check(self.L.adder_player_display_device(self.h, out.data_ptr(), None), 0)
            return out
        out = np.empty(self.shape, self.dtype)
        self._check(self.L.adder_player_display(self.h, out.ctypes.data), 0)
        return out


def play_file(path, playback_fps=60.0, out="f64", batch_events=1 << 20, max_batch_frames=64, device_id=0):
    """adder_video_player: yields the frames a raw .adder file shows at playback_fps (60.0 is the reference's CLI
    default), one [height, width, channels] numpy array at a time, in bounded memory: the file is read in batches of
    batch_events wire records and a batch may show at most max_batch_frames frames; one that would show more
    (E_OUT_CAPACITY, nothing changed) is halved and played again.  A batch of one record shows at most one frame.
    A bad event (see include/adder_player.h) ends the run: the frames before it are yielded, then
    AdderHipError(E_BAD_EVENT) is raised, its .index the event's index in the file."""
    with open(path, "rb") as f:
        meta, hb, eb = parse_header(f.read(64))
        f.seek(hb)
        pl = HipPlayer(playback_fps=playback_fps, out=out, device_id=device_id, **meta)
        try:
            n_in = 0
            pending = b""
            ended = False
            while not ended:
                if not pending:
                    pending = f.read(batch_events * eb)
                    if len(pending) < eb:
                        # a file without an EOF record: the short read ends the stream, its check is still made
                        for fr in pl.finish().cpu().numpy():
                            yield fr
                        break
                n = min(len(pending) // eb, batch_events)
                while True:
                    try:
                        frames = pl.play_wire(pending[: n * eb], max_frames=max(max_batch_frames, 1))
                        break
                    except N.AdderHipError as e:
                        if e.code != N.E_OUT_CAPACITY or n == 1:
                            raise
                        n = (n + 1) // 2
                for fr in frames:
                    yield fr
                if pl.bad_index is not None:
                    err = N.AdderHipError(E_BAD_EVENT, f"event {n_in + pl.bad_index} of {path} lies outside the plane")
                    err.index = n_in + pl.bad_index
                    raise err
                n_in += pl.consumed
                ended = pl.consumed < n
                pending = pending[n * eb:]
                if len(pending) < eb:
                    pending = b""
        finally:
            pl.close()
