"""HipVizPlayer: ctypes binding of the adder-viz player in libadder_hip.so (include/adder_viz_player.h), and
viz_play_file, the reference's interactive player (adder-viz/src/player/adder.rs) on a raw .adder file: the frames it
would show, streamed through the device batch by batch.

Inputs are numpy arrays (host forms of the C-ABI) or torch device tensors (device forms): AdderEvents (EVENT_DTYPE, or
their bytes) or the 9 / 11-byte wire records of a .adder body.  Frames are [n][height][width][channels] uint8 in one
of two forms: "popped" (the popped frame, None as 0: the reference's write_frame_bytes) or "running" (the player's
running_frame, what it shows).
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import player as _player

ABI_VERSION = 1
POPPED, RUNNING = 0, 1
FORMS = {"popped": POPPED, "running": RUNNING}
E_BAD_EVENT = -16
NO_BAD_EVENT = (1 << 64) - 1


class AdderVizPlayerParams(C.Structure):
    """include/adder_viz_player.h::AdderVizPlayerParams"""
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("width", C.c_uint16),
        ("height", C.c_uint16),
        ("channels", C.c_uint8),
        ("codec_version", C.c_uint8),
        ("time_mode", C.c_uint8),
        ("has_buffer_limit", C.c_uint8),
        ("buffer_limit", C.c_uint32),
        ("tps", C.c_uint32),
        ("ref_interval", C.c_uint32),
        ("delta_t_max", C.c_uint32),
        ("output_fps", C.c_float),
        ("source_camera", C.c_uint32),
        ("ring_frames", C.c_uint32),
        ("device_id", C.c_int32),
        ("view_mode", C.c_uint8),
        ("source_type", C.c_uint8),
        ("reserved0", C.c_uint16),
        ("practical_d_max", C.c_float),
    ]


_vp, _i32, _u64, _u32 = C.c_void_p, C.c_int, C.c_uint64, C.c_uint32
_pu64 = C.POINTER(C.c_uint64)
SYMBOLS = {
    "adder_viz_player_create": (_i32, [C.POINTER(AdderVizPlayerParams), C.POINTER(_vp)]),
    "adder_viz_player_destroy": (None, [_vp]),
    "adder_viz_player_reset": (_i32, [_vp]),
    "adder_viz_player_last_error": (C.c_char_p, [_vp]),
    "adder_viz_player_tpf": (_u32, [_vp]),
    "adder_viz_player_frames_written": (C.c_int64, [_vp]),
    "adder_viz_player_set_buffer_limit": (_i32, [_vp, _i32, _u32]),
    "adder_viz_player_ingest_device": (_i32, [_vp, _vp, _u64, _i32, _vp, _u64, _pu64, _vp, _pu64, _vp]),
    "adder_viz_player_ingest_wire_device": (_i32, [_vp, _vp, _u64, _i32, _vp, _u64, _pu64, _vp, _pu64, _pu64, _vp]),
    "adder_viz_player_finish_device": (_i32, [_vp, _i32, _vp, _u64, _pu64, _vp, _vp]),
    "adder_viz_player_ingest": (_i32, [_vp, _vp, _u64, _i32, _vp, _u64, _pu64, _vp, _pu64]),
    "adder_viz_player_ingest_wire": (_i32, [_vp, _vp, _u64, _i32, _vp, _u64, _pu64, _vp, _pu64, _pu64]),
    "adder_viz_player_finish": (_i32, [_vp, _i32, _vp, _u64, _pu64, _vp]),
    "adder_viz_player_running_frame": (_i32, [_vp, _vp]),
    "adder_viz_player_detect_features": (_i32, [_vp, _i32]),
    "adder_viz_player_features": (_i32, [_vp, _vp, _u64, _pu64]),
    "adder_viz_player_frame_features": (_i32, [_vp, _vp, _vp, _vp, _u64, _pu64]),
    "adder_viz_player_running_intensities": (_i32, [_vp, _vp]),
    "adder_viz_player_running_intensities_device": (_i32, [_vp, _vp, _vp]),
    "adder_viz_features_host": (_i32, [_vp, _u32, _u64, _vp, _i32, _vp, _vp]),
    "adder_viz_overlay_host": (_i32, [_u32, _u32, _vp, _vp, _vp, _u32, _vp, _vp]),
    "adder_viz_schedule_host": (C.c_int64, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _i32, _u32, _i32, _vp, _vp, _u64]),
}


def load():
    return N.bind(SYMBOLS)


def schedule_host(row, frm, to, last_filled, rows, row_units, buffer_limit, finish=False):
    """The library's pop schedule on the host (the function the schedule kernel runs), for one whole stream fed to a
    fresh context: per event its row, fill range (from, to] and L (-1: not checked) -> (P of each popped frame, local
    to the stream, int64; flushed marks uint8)."""
    arr = [np.ascontiguousarray(a, dtype=np.int32) for a in (row, frm, to, last_filled)]
    n = len(arr[0])
    cap = int(max([int(a.max()) for a in arr[2:]] + [0])) + 3 if n else 3
    pops, fl = np.zeros(cap, np.int64), np.zeros(cap, np.uint8)
    k = load().adder_viz_schedule_host(*[a.ctypes.data if n else None for a in arr], n, rows, row_units,
                                       0 if buffer_limit is None else 1, buffer_limit or 0, 1 if finish else 0,
                                       pops.ctypes.data, fl.ctypes.data, cap)
    if k < 0:
        raise ValueError("adder_viz_schedule_host refused its arguments")
    return pops[:k], fl[:k]


def features_host(pops, marks, w0=0):
    """Where the schedule meets detection, on the host (the functions the kernels run): pops = the local index of the
    event after which each frame is popped, marks = FAST corners per event -> (marks without the first event of every
    period, uint8; frames_written of each event's period, int32)."""
    pops = np.ascontiguousarray(pops, dtype=np.int32)
    marks = np.ascontiguousarray(marks, dtype=np.uint8)
    out, w = np.zeros(len(marks), np.uint8), np.zeros(len(marks), np.int32)
    rc = load().adder_viz_features_host(pops.ctypes.data if len(pops) else None, len(pops), len(marks),
                                        marks.ctypes.data, w0, out.ctypes.data, w.ctypes.data)
    if rc != N.OK:
        raise ValueError("adder_viz_features_host refused its arguments")
    return out, w


def overlay_host(some, val, stamps, running):
    """The hand-out's running-frame rule on the host: some / val [n_pops, units] (the popped frames), stamps = (unit,
    frame k) pairs in any order, running = the running frame before -> (RUNNING-form frames, the running frame after)."""
    some = np.ascontiguousarray(some, dtype=np.uint8)
    val = np.ascontiguousarray(val, dtype=np.uint8)
    n_pops, units = some.shape
    keys = np.sort(np.array([(int(u) << 32) | int(k) for u, k in stamps], np.uint64))
    run = np.array(running, np.uint8).reshape(-1).copy()
    frames = np.zeros((n_pops, units), np.uint8)
    rc = load().adder_viz_overlay_host(units, n_pops, some.ctypes.data, val.ctypes.data,
                                       keys.ctypes.data if len(keys) else None, len(keys), run.ctypes.data,
                                       frames.ctypes.data)
    if rc != N.OK:
        raise ValueError("adder_viz_overlay_host refused its arguments")
    return frames, run


class HipVizPlayer(N.Handle):
    """The player's state on one device.  Every ingest call continues the stream where the last one stopped and
    returns the frames popped during it; finish() ends the stream.

    After a call: .pop_index holds, per returned frame, the global index of the event after which it was popped (-1:
    before the first); .bad_index is the index (within that call's input) of the event that stopped it, or None;
    .consumed is the number of wire records before an EOF record (all of them when there is none).

    A call whose frames do not fit max_frames raises AdderHipError(E_OUT_CAPACITY) with .needed = the count, and
    changes nothing."""
    DESTROY = "adder_viz_player_destroy"

    def __init__(self, width, height, channels=1, *, tps, ref_interval, delta_t_max, output_fps, codec_version=2,
                 time_mode=N.TIME_DELTA_T, source_camera=0, buffer_limit=60, view_mode=0, source_type=0,
                 practical_d_max=0.0, ring_frames=0, form="running", device_id=0):
        self.L = load()
        p = AdderVizPlayerParams(
            abi_version=ABI_VERSION, width=width, height=height, channels=channels, codec_version=codec_version,
            time_mode=time_mode, has_buffer_limit=0 if buffer_limit is None else 1, buffer_limit=buffer_limit or 0,
            tps=tps, ref_interval=ref_interval, delta_t_max=delta_t_max,
            output_fps=-1.0 if output_fps is None else float(output_fps), source_camera=source_camera,
            ring_frames=ring_frames, device_id=device_id, view_mode=view_mode, source_type=source_type,
            practical_d_max=practical_d_max)
        h = C.c_void_p()
        rc = self.L.adder_viz_player_create(C.byref(p), C.byref(h))
        if rc != N.OK:
            raise N.AdderHipError(rc, (self.L.adder_viz_player_last_error(None) or b"").decode())
        self.h, self.params = h, p
        self.form = FORMS.get(form, form)
        self.record_bytes = 9 if channels == 1 else 11
        self.shape = (height, width, channels)
        self.units = height * width * channels
        self.bad_index, self.consumed, self.pop_index = None, 0, np.zeros(0, np.int64)

    def reset(self):
        self._check(self.L.adder_viz_player_reset(self.h), 0)

    @property
    def tpf(self):
        return self.L.adder_viz_player_tpf(self.h)

    @property
    def frames_written(self):
        return self.L.adder_viz_player_frames_written(self.h)

    def set_buffer_limit(self, buffer_limit):
        rc = self.L.adder_viz_player_set_buffer_limit(self.h, 0 if buffer_limit is None else 1, buffer_limit or 0)
        self._check(rc, 0)

    def detect_features(self, on):
        """Framer::detect_features; may be switched between any two calls (clears the carried last event)."""
        self._check(self.L.adder_viz_player_detect_features(self.h, 1 if on else 0), 0)

    def features(self):
        """The features of the last ingest call: FEATURE_DTYPE records in stream order, index = the global stream index."""
        count = C.c_uint64(0)
        self.L.adder_viz_player_features(self.h, None, 0, C.byref(count))
        out = np.zeros(count.value, N.FRAMER_FEATURE_DTYPE)
        if count.value:
            self._check(self.L.adder_viz_player_features(self.h, out.ctypes.data, count.value, C.byref(count)), 0)
        return out

    def frame_features(self):
        """One FeatureInterval per frame of the last ingest / finish call: [(end_ts, [n, 2] uint16 {x, y})].
        .features_error holds the message once a feature could not be filed (the reference would have panicked)."""
        n = len(self.pop_index)
        pairs = C.c_uint64(0)
        end_ts, off = np.zeros(max(n, 1), np.uint64), np.zeros(n + 1, np.uint64)
        self.L.adder_viz_player_frame_features(self.h, end_ts.ctypes.data, off.ctypes.data, None, 0, C.byref(pairs))
        xy = np.zeros((max(pairs.value, 1), 2), np.uint16)
        rc = self.L.adder_viz_player_frame_features(self.h, end_ts.ctypes.data, off.ctypes.data, xy.ctypes.data,
                                                    pairs.value, C.byref(pairs))
        self.features_error = None
        if rc == N.E_BAD_PARAMS:
            self.features_error = (self.L.adder_viz_player_last_error(self.h) or b"").decode()
        else:
            self._check(rc, 0)
        return [(int(end_ts[j]), xy[int(off[j]): int(off[j + 1])].copy()) for j in range(n)]

    def running_intensities(self):
        """FrameSequence::get_running_intensities: [height, width, channels] uint8"""
        out = np.empty(self.shape, np.uint8)
        self._check(self.L.adder_viz_player_running_intensities(self.h, out.ctypes.data), 0)
        return out

    def running_frame(self):
        out = np.empty(self.shape, np.uint8)
        self._check(self.L.adder_viz_player_running_frame(self.h, out.ctypes.data), 0)
        return out

    def _check(self, rc, needed):
        if rc not in (N.OK, E_BAD_EVENT):
            err = N.AdderHipError(rc, (self.L.adder_viz_player_last_error(self.h) or b"").decode())
            err.needed = needed
            raise err

    def ingest(self, events, max_frames=None, stream=None, form=None):
        """AdderEvents: a numpy EVENT_DTYPE array (host form) or a torch CUDA tensor of their bytes (device form).
        -> the frames popped during this batch (numpy array / CUDA tensor), [n, height, width, channels]."""
        if isinstance(events, np.ndarray):
            ev = np.ascontiguousarray(events, dtype=N.EVENT_DTYPE)
            return self._call(self.L.adder_viz_player_ingest, ev, len(ev), max_frames, None, False, form, False)
        n = events.numel() * events.element_size() // 12
        return self._call(self.L.adder_viz_player_ingest_device, events, n, max_frames, stream, False, form, True)

    def ingest_wire(self, records, max_frames=None, stream=None, form=None):
        """Wire records (the body of a .adder file): numpy uint8 / bytes (host form) or a uint8 CUDA tensor."""
        rb = self.record_bytes
        if isinstance(records, (bytes, bytearray, memoryview, np.ndarray)):
            w = np.frombuffer(records, np.uint8) if not isinstance(records, np.ndarray) else \
                np.ascontiguousarray(records).view(np.uint8).reshape(-1)
            return self._call(self.L.adder_viz_player_ingest_wire, w, w.size // rb, max_frames, None, True, form, False)
        n = records.numel() * records.element_size() // rb
        return self._call(self.L.adder_viz_player_ingest_wire_device, records, n, max_frames, stream, True, form, True)

    def finish(self, max_frames=None, form=None, device=False):
        """The end of the stream: the frames the reference's flush loop shows."""
        return self._call(self.L.adder_viz_player_finish_device if device else self.L.adder_viz_player_finish, None, 0,
                          max_frames, None, False, form, device, finish=True)

    def _call(self, fn, data, n, max_frames, stream, wire, form, device, finish=False):
        form = self.form if form is None else FORMS.get(form, form)
        room = 16 if max_frames is None else max_frames
        n_frames, bad, consumed = C.c_uint64(0), C.c_uint64(NO_BAD_EVENT), C.c_uint64(n)
        if device:
            import torch
            dev = data.device if data is not None else f"cuda:{self.params.device_id}"
            mk = lambda k: torch.empty((k,) + self.shape, dtype=torch.uint8, device=dev)
            ptr = lambda t: t.data_ptr()
        else:
            mk = lambda k: np.empty((k,) + self.shape, np.uint8)
            ptr = lambda t: t.ctypes.data
        while True:
            out, pops = mk(max(room, 1)), np.zeros(max(room, 1), np.int64)
            args = [self.h]
            if not finish:
                args += [(ptr(data) if n else None), n]
            args += [form, ptr(out), room, C.byref(n_frames), pops.ctypes.data]
            if not finish:
                args.append(C.byref(bad))
                if wire:
                    args.append(C.byref(consumed))
            if device:
                args.append(C.c_void_p(stream) if stream else None)
            rc = fn(*args)
            # nothing changed: again, with the room it asks for (a needed count of 0 is the ring's error)
            if rc == N.E_OUT_CAPACITY and max_frames is None and n_frames.value > room:
                room = n_frames.value
                continue
            break
        self._check(rc, n_frames.value)
        self.bad_index = None if bad.value == NO_BAD_EVENT else bad.value
        self.consumed = consumed.value
        self.pop_index = pops[: n_frames.value].copy()
        return out[: n_frames.value]


def reconstructed_frame_rate(tps, ref_interval, source_camera, playback_speed=1.0):
    """adder.rs:263-269, in f32: tps / ref_interval for framed cameras, else 60; divided by the playback speed."""
    f32 = np.float32
    rate = f32(tps) / f32(ref_interval) if source_camera <= 5 else f32(60.0)
    return float(rate / f32(playback_speed))


def parse_header(buf):
    """-> (meta dict for HipVizPlayer, header bytes, event bytes) of a raw .adder stream of codec version 0..3"""
    b = bytes(buf[:64])
    meta, hb, eb = _player.parse_header(b)
    meta["codec_version"] = b[5]
    meta["delta_t_max"] = int.from_bytes(b[19:23], "big")
    return meta, hb, eb


def viz_play_file(path, buffer_limit=60, playback_speed=1.0, form="running", batch_events=1 << 20, view_mode=0,
                  max_records=None, device_id=0, detect_features=False):
    """The adder-viz player on a raw .adder file: yields the frames it shows, one [height, width, channels] uint8 array
    at a time, the flush at the end of the file included.  The file is read in batches of batch_events wire records (a
    batch whose units run past the pending ring is fed in halves);
    max_records cuts the stream short (the cut is then its end).  A bad event ends the run: the frames before it are
    yielded, then AdderHipError(E_BAD_EVENT) is raised, its .index the event's index in the file.
    detect_features: the player's feature detection; the "running" frames then carry the crosses, and every item
    yielded is (frame, (end_ts, [n, 2] uint16 {x, y})): the frame with the FeatureInterval popped with it."""
    with open(path, "rb") as f:
        meta, hb, eb = parse_header(f.read(64))
        f.seek(hb)
        fps = reconstructed_frame_rate(meta["tps"], meta["ref_interval"], meta["source_camera"], playback_speed)
        pl = HipVizPlayer(output_fps=fps, buffer_limit=buffer_limit, view_mode=view_mode, form=form,
                          device_id=device_id, **meta)
        if detect_features:
            pl.detect_features(True)
        with_intervals = (lambda frames: zip(frames, pl.frame_features())) if detect_features else (lambda frames: frames)
        try:
            n_in = 0
            while True:
                want = batch_events if max_records is None else min(batch_events, max_records - n_in)
                data = f.read(want * eb) if want > 0 else b""
                n = len(data) // eb
                if n == 0:
                    break
                at, take, ended = 0, n, False
                while at < n and not ended:
                    take = min(take, n - at)
                    try:
                        frames = pl.ingest_wire(data[at * eb: (at + take) * eb])
                    except N.AdderHipError as e:
                        # some unit of these records runs further ahead than the pending ring holds (nothing
                        # changed): fewer records at a time let the pops in between make room
                        if e.code != N.E_OUT_CAPACITY or take == 1:
                            raise
                        take = (take + 1) // 2
                        continue
                    for fr in with_intervals(frames):
                        yield fr
                    if pl.bad_index is not None:
                        err = N.AdderHipError(E_BAD_EVENT,
                                              f"event {n_in + pl.bad_index} of {path} lies outside the plane")
                        err.index = n_in + pl.bad_index
                        raise err
                    n_in += pl.consumed
                    ended = pl.consumed < take
                    at += take
                if ended:
                    break
            for fr in with_intervals(pl.finish()):
                yield fr
        finally:
            pl.close()
