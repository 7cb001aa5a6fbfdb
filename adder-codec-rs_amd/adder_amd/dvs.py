"""HipDvs: ctypes binding of the ADDER -> DVS conversion in libadder_hip.so (include/adder_dvs.h), and
adder_to_dvs_file, the reference's adder-to-dvs tool (a raw .adder file -> Prophesee .dat or text) streamed through
the device batch by batch.

Inputs are numpy arrays (host forms of the C-ABI) or torch device tensors (device forms): AdderEvents (EVENT_DTYPE,
or their bytes) or the 9 / 11-byte wire records of a .adder body.  Outputs are DVS_EVENT_DTYPE (the full time) or
DAT_DTYPE (the .dat record).
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

    @classmethod
    def from_header(cls, buf, theta=0.01, device_id=0):
        meta, _, _ = parse_header(buf)
        return cls(theta=theta, device_id=device_id, **meta)

    def reset(self):
        self._check(self.L.adder_dvs_reset(self.h))

    def _check(self, rc):
        if rc not in (N.OK, E_BAD_EVENT):
            raise N.AdderHipError(rc, (self.L.adder_dvs_last_error(self.h) or b"").decode())

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
                      batch_records=1 << 24, device_id=0):
    """adder-to-dvs: a raw .adder file -> DVS events, Prophesee .dat (binary) or "t x y p" lines (text=True).
    The file is streamed through the device in batches of batch_records wire records.  reorder (binary only):
    the whole output is kept on the device and written after a stable sort by 32-bit t.  date: the header's
    "YYYY-mm-dd HH:MM:SS" (default: now).  A bad event (see include/adder_dvs.h) ends the run like the reference's:
    the output before it is written (with reorder: none of it) and AdderHipError(E_BAD_EVENT) is raised, its
    .index the event's index in the file.  -> dict(events_in, events_out)."""
    if date is None:
        date = datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")
    reorder = reorder and not text  # the queue is only fed in binary mode (main.rs:501-524)
    fmt = OUT_EVENTS if text else OUT_DAT
    with open(in_path, "rb") as f:
        meta, hb, eb = parse_header(f.read(64))
        f.seek(hb)
        dvs = HipDvs(theta=theta, device_id=device_id, **meta)
        n_in = n_out = 0
        kept = []
        bad = None
        with open(out_path, "wb") as g:
            g.write(header_bytes(meta["width"], meta["height"], date, binary=not text))
            while True:
                buf = f.read(batch_records * eb)
                n = len(buf) // eb
                if n == 0:
                    break
                if reorder:
                    import torch
                    d = torch.frombuffer(bytearray(buf[: n * eb]), dtype=torch.uint8).to(f"cuda:{device_id}")
                    recs = dvs.convert_wire(d, fmt)
                    kept.append(recs)
                else:
                    recs = dvs.convert_wire(buf[: n * eb], fmt)
                    g.write(format_text(recs) if text else recs.tobytes())
                n_in += dvs.consumed if dvs.bad_index is None else dvs.bad_index
                n_out += len(recs) if not reorder else recs.numel() // 8
                if dvs.bad_index is not None:
                    bad = n_in
                    break
                if dvs.consumed < n or n < batch_records:
                    break
            if reorder and bad is None and n_out:
                import torch
                allr = torch.cat(kept)
                dvs.sort(allr, OUT_DAT)
                g.write(allr.cpu().numpy().tobytes())
        dvs.close()
    if bad is not None:
        err = N.AdderHipError(E_BAD_EVENT, f"event {bad} of {in_path} cannot be converted to DVS")
        err.index = bad
        raise err
    return dict(events_in=n_in, events_out=n_out)
