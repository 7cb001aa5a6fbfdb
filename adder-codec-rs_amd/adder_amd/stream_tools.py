"""HipStreamMigrator / HipStreamInfo: ctypes binding of the stream tools in libadder_hip.so (include/adder_stream.h),
and the reference's two tools over files: migrate_file (migrate_raw_v0_v1_to_v2: a raw .adder file rewritten in
another time mode) and adder_info_file (adder-info: the report, with the realised dynamic range on request), each
streamed through the device batch by batch.

Inputs are numpy arrays (host forms of the C-ABI) or torch device tensors (device forms): AdderEvents (EVENT_DTYPE,
or their bytes) or the 9 / 11-byte wire records of a .adder body.
"""
import ctypes as C
import os

import numpy as np

from . import _native as N

ABI_VERSION = 1
E_BAD_EVENT = -20
NO_BAD_EVENT = (1 << 64) - 1
TIME_MODES = {"delta_t": N.TIME_DELTA_T, "absolute": N.TIME_ABSOLUTE_T, "mixed": N.TIME_MIXED}


class AdderStreamParams(C.Structure):
    """include/adder_stream.h::AdderStreamParams"""
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("width", C.c_uint16),
        ("height", C.c_uint16),
        ("channels", C.c_uint8),
        ("codec_version", C.c_uint8),
        ("time_mode", C.c_uint8),
        ("out_time_mode", C.c_uint8),
        ("ref_interval", C.c_uint32),
        ("source_camera", C.c_uint32),
        ("tps", C.c_uint32),
        ("delta_t_max", C.c_uint32),
        ("device_id", C.c_int32),
    ]


_vp, _i32, _u64, _sz, _f64 = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t, C.c_double
_pu64, _pu32, _pf64 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
_pp = C.POINTER(AdderStreamParams)
SYMBOLS = {
    "adder_stream_parse_header": (_i32, [_vp, _sz, _pp, _pu32, _pu32]),
    "adder_stream_migrated_header": (_sz, [_vp, _sz, C.c_uint32, _vp, _sz]),
    "adder_stream_create": (_i32, [_pp, C.POINTER(_vp)]),
    "adder_stream_destroy": (None, [_vp]),
    "adder_stream_reset": (_i32, [_vp]),
    "adder_stream_last_error": (C.c_char_p, [_vp]),
    "adder_stream_migrate_device": (_i32, [_vp, _vp, _u64, _vp, _pu64, _vp]),
    "adder_stream_migrate_wire_device": (_i32, [_vp, _vp, _u64, _vp, _pu64, _pu64, _vp]),
    "adder_stream_migrate_host": (_i32, [_vp, _vp, _u64, _vp, _pu64]),
    "adder_stream_migrate_wire_host": (_i32, [_vp, _vp, _u64, _vp, _pu64, _pu64]),
    "adder_stream_info_device": (_i32, [_vp, _vp, _u64, _pu64, _vp]),
    "adder_stream_info_wire_device": (_i32, [_vp, _vp, _u64, _pu64, _pu64, _vp]),
    "adder_stream_info_host": (_i32, [_vp, _vp, _u64, _pu64]),
    "adder_stream_info_wire_host": (_i32, [_vp, _vp, _u64, _pu64, _pu64]),
    "adder_stream_info_range": (_i32, [_vp, _pf64, _pf64, _pu64]),
    "adder_stream_format_report": (_sz, [_pp, C.c_uint32, _u64, _u64, _i32, _f64, _f64, _vp, _sz]),
}
META_KEYS = ("width", "height", "channels", "codec_version", "time_mode", "ref_interval", "source_camera", "tps",
             "delta_t_max")


def load():
    return N.bind(SYMBOLS)


def _params(meta, out_time_mode=None, device_id=0):
    return AdderStreamParams(abi_version=ABI_VERSION, device_id=device_id,
                             out_time_mode=meta["time_mode"] if out_time_mode is None else out_time_mode,
                             **{k: meta[k] for k in META_KEYS})


def parse_header(buf):
    """-> (meta dict with META_KEYS; header bytes; event bytes) of a raw .adder stream of codec version 0..3."""
    b = bytes(buf[:64])
    p, hb, eb = AdderStreamParams(), C.c_uint32(0), C.c_uint32(0)
    rc = load().adder_stream_parse_header(b, len(b), C.byref(p), C.byref(hb), C.byref(eb))
    if rc != N.OK:
        raise N.AdderHipError(rc, "not a raw .adder header of codec version 0..3 (compressed streams: decode them "
                                  "with adder_compressed_decode and use the event entry points)")
    return {k: getattr(p, k) for k in META_KEYS}, hb.value, eb.value


def migrated_header(header, time_mode):
    """The input's header with time_mode set and the codec version raised to 2 where it was below."""
    b = bytes(header[:64])
    out = C.create_string_buffer(64)
    n = load().adder_stream_migrated_header(b, len(b), time_mode, out, 64)
    if n == 0:
        raise N.AdderHipError(N.E_BAD_PARAMS, "not a raw .adder header, or no such time mode")
    return out.raw[:n]


def format_report(meta, header_bytes, file_bytes, n_events, dynamic_range=False, min_intensity=0.0,
                  max_intensity=0.0):
    """adder-info's text for a stream with this metadata (main.rs:47-66, 137-147)."""
    p = _params(meta)
    args = (C.byref(p), header_bytes, file_bytes, n_events, 1 if dynamic_range else 0, min_intensity, max_intensity)
    L = load()
    n = L.adder_stream_format_report(*args, None, 0)
    buf = C.create_string_buffer(n)
    L.adder_stream_format_report(*args, buf, n)
    return buf.raw[:n].decode()


class _Handle(N.Handle):
    """One adder_stream handle.  After a call: .bad_index is the index (within that call's input) of the event that
    stopped it, or None -- the events before it are applied, nothing after it is; .consumed is the number of wire
    records before an EOF record (all of them when there is none)."""
    DESTROY = "adder_stream_destroy"

    def __init__(self, meta, out_time_mode, device_id):
        self.L = load()
        p = _params(meta, out_time_mode, device_id)
        h = C.c_void_p()
        rc = self.L.adder_stream_create(C.byref(p), C.byref(h))
        if rc != N.OK:
            raise N.AdderHipError(rc, (self.L.adder_stream_last_error(None) or b"").decode())
        self.h, self.params, self.meta = h, p, dict(meta)
        self.record_bytes = 9 if meta["channels"] == 1 else 11
        self.bad_index, self.consumed = None, 0

    def reset(self):
        self._done(self.L.adder_stream_reset(self.h), C.c_uint64(NO_BAD_EVENT), 0)

    def _done(self, rc, bad, consumed):
        if rc not in (N.OK, E_BAD_EVENT):
            raise N.AdderHipError(rc, (self.L.adder_stream_last_error(self.h) or b"").decode())
        self.bad_index = None if bad.value == NO_BAD_EVENT else bad.value
        self.consumed = consumed

    def _wire_host(self, records):
        if isinstance(records, np.ndarray):
            return np.ascontiguousarray(records).view(np.uint8).reshape(-1)
        return np.frombuffer(records, np.uint8)


def _meta(width, height, channels, codec_version, time_mode, ref_interval, source_camera, tps, delta_t_max):
    return dict(width=width, height=height, channels=channels, codec_version=codec_version, time_mode=time_mode,
                ref_interval=ref_interval, source_camera=source_camera, tps=tps, delta_t_max=delta_t_max)


class HipStreamMigrator(_Handle):
    """Per-unit migration state on one device: DeltaT -> AbsoluteT (migrate_v2), AbsoluteT -> DeltaT (its inverse),
    anything else passes events through.  Every call continues the stream where the last one stopped."""

    def __init__(self, width, height, channels=1, *, codec_version=2, time_mode=N.TIME_DELTA_T,
                 out_time_mode=N.TIME_ABSOLUTE_T, ref_interval=255, source_camera=0, tps=0, delta_t_max=0,
                 device_id=0):
        super().__init__(_meta(width, height, channels, codec_version, time_mode, ref_interval, source_camera, tps,
                               delta_t_max), out_time_mode, device_id)

    @classmethod
    def from_header(cls, buf, out_time_mode, device_id=0):
        meta, _, _ = parse_header(buf)
        return cls(out_time_mode=out_time_mode, device_id=device_id, **meta)

    def migrate(self, events, out=None, stream=None):
        """AdderEvents: a numpy EVENT_DTYPE array (host form; -> the migrated events before the bad index) or a torch
        CUDA tensor of their bytes (device form; -> `out`, default a new tensor, `out=events` migrates in place)."""
        bad = C.c_uint64(0)
        if isinstance(events, np.ndarray):
            ev = np.ascontiguousarray(events, dtype=N.EVENT_DTYPE)
            res = np.zeros(len(ev), N.EVENT_DTYPE)
            rc = self.L.adder_stream_migrate_host(self.h, ev.ctypes.data if len(ev) else None, len(ev),
                                                  res.ctypes.data if len(ev) else None, C.byref(bad))
            self._done(rc, bad, len(ev))
            return res[: len(ev) if self.bad_index is None else self.bad_index]
        import torch
        n = events.numel() * events.element_size() // 12
        if out is None:
            out = torch.empty_like(events)
        rc = self.L.adder_stream_migrate_device(self.h, events.data_ptr() if n else None, n,
                                                out.data_ptr() if n else None, C.byref(bad),
                                                C.c_void_p(stream) if stream else None)
        self._done(rc, bad, n)
        return out

    def migrate_wire(self, records, out=None, stream=None):
        """Wire records: numpy uint8 / bytes (host form; -> the migrated bytes before the bad / EOF index) or a uint8
        CUDA tensor (device form; -> `out`)."""
        rb = self.record_bytes
        bad, consumed = C.c_uint64(0), C.c_uint64(0)
        if isinstance(records, (bytes, bytearray, memoryview, np.ndarray)):
            w = self._wire_host(records)
            n = w.size // rb
            res = np.zeros(n * rb, np.uint8)
            rc = self.L.adder_stream_migrate_wire_host(self.h, w.ctypes.data if n else None, n,
                                                       res.ctypes.data if n else None, C.byref(bad), C.byref(consumed))
            self._done(rc, bad, consumed.value)
            done = self.consumed if self.bad_index is None else min(self.bad_index, self.consumed)
            return res[: done * rb].tobytes()
        import torch
        n = records.numel() * records.element_size() // rb
        if out is None:
            out = torch.empty_like(records)
        rc = self.L.adder_stream_migrate_wire_device(self.h, records.data_ptr() if n else None, n,
                                                     out.data_ptr() if n else None, C.byref(bad), C.byref(consumed),
                                                     C.c_void_p(stream) if stream else None)
        self._done(rc, bad, consumed.value)
        return out


class HipStreamInfo(_Handle):
    """adder-info's dynamic-range fold on one device; .range() is (min_intensity, max_intensity, events folded)."""

    def __init__(self, width, height, channels=1, *, codec_version=2, time_mode=N.TIME_DELTA_T, ref_interval=255,
                 source_camera=0, tps=0, delta_t_max=0, device_id=0):
        super().__init__(_meta(width, height, channels, codec_version, time_mode, ref_interval, source_camera, tps,
                               delta_t_max), None, device_id)

    @classmethod
    def from_header(cls, buf, device_id=0):
        meta, _, _ = parse_header(buf)
        return cls(device_id=device_id, **meta)

    def fold(self, events, stream=None):
        """AdderEvents: a numpy EVENT_DTYPE array (host form) or a torch CUDA tensor of their bytes (device form)."""
        bad = C.c_uint64(0)
        if isinstance(events, np.ndarray):
            ev = np.ascontiguousarray(events, dtype=N.EVENT_DTYPE)
            rc = self.L.adder_stream_info_host(self.h, ev.ctypes.data if len(ev) else None, len(ev), C.byref(bad))
            self._done(rc, bad, len(ev))
        else:
            n = events.numel() * events.element_size() // 12
            rc = self.L.adder_stream_info_device(self.h, events.data_ptr() if n else None, n, C.byref(bad),
                                                 C.c_void_p(stream) if stream else None)
            self._done(rc, bad, n)
        return self.range()

    def fold_wire(self, records, stream=None):
        rb = self.record_bytes
        bad, consumed = C.c_uint64(0), C.c_uint64(0)
        if isinstance(records, (bytes, bytearray, memoryview, np.ndarray)):
            w = self._wire_host(records)
            n = w.size // rb
            rc = self.L.adder_stream_info_wire_host(self.h, w.ctypes.data if n else None, n, C.byref(bad),
                                                    C.byref(consumed))
        else:
            n = records.numel() * records.element_size() // rb
            rc = self.L.adder_stream_info_wire_device(self.h, records.data_ptr() if n else None, n, C.byref(bad),
                                                      C.byref(consumed), C.c_void_p(stream) if stream else None)
        self._done(rc, bad, consumed.value)
        return self.range()

    def range(self):
        lo, hi, n = C.c_double(0), C.c_double(0), C.c_uint64(0)
        self.L.adder_stream_info_range(self.h, C.byref(lo), C.byref(hi), C.byref(n))
        return lo.value, hi.value, n.value

    def report(self, header_bytes, file_bytes, n_events, dynamic_range=True):
        lo, hi, _ = self.range()
        return format_report(self.meta, header_bytes, file_bytes, n_events, dynamic_range, lo, hi)


def _bad(index, path, what):
    err = N.AdderHipError(E_BAD_EVENT, f"event {index} of {path} {what}")
    err.index = index
    return err


def _batches(f, eb, batch_records):
    while True:
        buf = f.read(batch_records * eb)
        n = len(buf) // eb
        if n == 0:
            return
        yield buf[: n * eb], n
        if n < batch_records:
            return


def migrate_file(in_path, out_path, time_mode, *, batch_records=1 << 24, device_id=0):
    """migrate_raw_v0_v1_to_v2: a raw .adder file rewritten with `time_mode` ("delta_t", "absolute", "mixed", or an
    ADDER_TIME_* value).  The body is streamed through the device in batches of batch_records wire records; the output
    ends with the 11-byte EOF record.  A bad event (see include/adder_stream.h) ends the run: the events before it
    and the EOF record are written and AdderHipError(E_BAD_EVENT) is raised, its .index the event's index in the
    file.  -> dict(events=the events written)."""
    if isinstance(time_mode, str):
        if time_mode.lower() not in TIME_MODES:
            raise ValueError("Invalid time mode")
        time_mode = TIME_MODES[time_mode.lower()]
    total, bad = 0, None
    with open(in_path, "rb") as f:
        head = f.read(64)
        _, hb, eb = parse_header(head)
        f.seek(hb)
        mig = HipStreamMigrator.from_header(head, time_mode, device_id)
        with open(out_path, "wb") as g:
            g.write(migrated_header(head, time_mode))
            for buf, n in _batches(f, eb, batch_records):
                g.write(mig.migrate_wire(buf))
                if mig.bad_index is not None:
                    bad = total + mig.bad_index
                    total = bad
                    break
                total += mig.consumed
                if mig.consumed < n:
                    break
            g.write(_eof())
        mig.close()
    if bad is not None:
        raise _bad(bad, in_path, "cannot be migrated")
    return dict(events=total)


def _eof():
    buf = np.zeros(16, np.uint8)
    n = N.load().adder_raw_eof(buf.ctypes.data)
    return buf[:n].tobytes()


def adder_info_file(path, dynamic_range=False, *, batch_records=1 << 24, device_id=0):
    """adder-info: the report of a raw .adder file as text.  The event count is the number of records in front of the
    EOF record, counted on the device; dynamic_range adds the fold over every event.  Compressed files are refused."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(64)
        meta, hb, eb = parse_header(head)
        f.seek(hb)
        info = HipStreamInfo.from_header(head, device_id)
        total = 0
        for buf, n in _batches(f, eb, batch_records):
            info.fold_wire(buf)
            if info.bad_index is not None:
                raise _bad(total + info.bad_index, path, "cannot be folded")
            total += info.consumed
            if info.consumed < n:
                break
        text = info.report(hb, size, total, dynamic_range)
        info.close()
    return text
