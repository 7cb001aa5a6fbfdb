"""HipProphesee: ctypes binding of the Prophesee .dat -> ADDER transcoder in libadder_hip.so
(include/adder_prophesee.h), and prophesee_to_adder_file, the reference's prophesee_to_adder tool streamed through
the device in chunks of records.

Records are the 8-byte body of a .dat file: numpy / bytes (host forms of the C-ABI) or uint8 torch CUDA tensors
(device forms).  Events come back as EVENT_DTYPE arrays (host) or uint8 CUDA tensors of whole AdderEvents (device).
"""
import ctypes as C
import os

import numpy as np

from . import _native as N
from .video import CRF, DEFAULT_CRF_QUALITY

ABI_VERSION = 1
E_BAD_RECORD, E_END_ASSERT, E_ORDER = -17, -18, -19
NO_CRF = -1
NO_BAD_RECORD = (1 << 64) - 1
VIEW_INTERVAL = 16666
SOURCE_TPS = 1000000
SOURCE_CAMERA_DVS = 6  # SourceCamera::Dvs
CODEC_VERSION = 3

RECORD_DTYPE = np.dtype([("t", "<u4"), ("data", "<i4")])  # a .dat record
EVENT_DTYPE_PPH = np.dtype([("t", "<u4"), ("x", "<u2"), ("y", "<u2"), ("p", "u1"), ("pad", "u1", (3,))])
assert RECORD_DTYPE.itemsize == 8 and EVENT_DTYPE_PPH.itemsize == 12


class AdderPropheseeHeader(C.Structure):
    """include/adder_prophesee.h::AdderPropheseeHeader"""
    _fields_ = [("width", C.c_uint16), ("height", C.c_uint16), ("header_bytes", C.c_uint32), ("ev_type", C.c_uint8),
                ("ev_size", C.c_uint8), ("header_lines", C.c_uint8), ("reserved0", C.c_uint8)]


class AdderPropheseeParams(C.Structure):
    """include/adder_prophesee.h::AdderPropheseeParams"""
    _fields_ = [("abi_version", C.c_uint32), ("width", C.c_uint16), ("height", C.c_uint16), ("ref_time", C.c_uint32),
                ("crf", C.c_int32), ("device_id", C.c_int32)]


_vp, _i32, _u64, _sz, _u32 = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t, C.c_uint32
_pu64, _pu32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
SYMBOLS = {
    "adder_prophesee_parse_header": (_i32, [_vp, _sz, _u64, C.POINTER(AdderPropheseeHeader)]),
    "adder_prophesee_decode": (None, [_vp, _u64, _vp]),
    "adder_prophesee_scan_groups": (_u64, [_vp, _u64, _pu32, _pu32, _pu64]),
    "adder_prophesee_create": (_i32, [C.POINTER(AdderPropheseeParams), C.POINTER(_vp)]),
    "adder_prophesee_destroy": (None, [_vp]),
    "adder_prophesee_reset": (_i32, [_vp]),
    "adder_prophesee_last_error": (C.c_char_p, [_vp]),
    "adder_prophesee_events_per_step": (_u64, [_vp]),
    "adder_prophesee_start": (_i32, [_vp, _vp, _u64, _pu64]),
    "adder_prophesee_push_device": (_i32, [_vp, _vp, _u64, _vp, _u64, _pu64, _pu64, _vp]),
    "adder_prophesee_push_host": (_i32, [_vp, _vp, _u64, _vp, _u64, _pu64, _pu64]),
    "adder_prophesee_finish_device": (_i32, [_vp, _vp, _u64, _pu64, _vp]),
    "adder_prophesee_finish_host": (_i32, [_vp, _vp, _u64, _pu64]),
    "adder_prophesee_state": (_i32, [_vp, _pu32, _pu32, _pu64, _pu64]),
    "adder_prophesee_pixel_state": (_i32, [_vp, _vp, _vp]),
    "adder_prophesee_running_intensities": (_i32, [_vp, _vp]),
    "adder_prophesee_exp": (C.c_double, [C.c_double]),
    "adder_prophesee_exp_host": (None, [_vp, _vp, _u64]),
    "adder_prophesee_exp_device": (_i32, [_vp, _vp, _u64, _i32]),
}


def load():
    return N.bind(SYMBOLS)


def exp(x):
    """The library's binary64 exp on the host (the routine the kernels evaluate): a float, or a float64 array."""
    if np.ndim(x) == 0:
        return load().adder_prophesee_exp(float(x))
    xs = np.ascontiguousarray(x, dtype=np.float64)
    ys = np.empty_like(xs)
    load().adder_prophesee_exp_host(xs.ctypes.data, ys.ctypes.data, xs.size)
    return ys


def exp_device(x, device_id=0):
    """The same routine evaluated by a kernel (self-test): float64 array in, float64 array out."""
    import torch
    xs = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(f"cuda:{device_id}")
    ys = torch.empty_like(xs)
    rc = load().adder_prophesee_exp_device(xs.data_ptr(), ys.data_ptr(), xs.numel(), device_id)
    if rc != N.OK:
        raise N.AdderHipError(rc, "device exp")
    return ys.cpu().numpy()


def parse_header(buf, file_size=None):
    """parse_header over the first bytes of a .dat file -> dict(width, height, header_bytes, ev_type, ev_size,
    header_lines).  file_size defaults to len(buf) (the whole file).  Raises AdderHipError: E_BAD_PARAMS where the
    reference refuses, E_OUT_CAPACITY when buf ends inside the header."""
    b = bytes(buf)
    h = AdderPropheseeHeader()
    rc = load().adder_prophesee_parse_header(b, len(b), len(b) if file_size is None else file_size, C.byref(h))
    if rc != N.OK:
        raise N.AdderHipError(rc, "not a Prophesee .dat header the reference accepts")
    return dict(width=h.width, height=h.height, header_bytes=h.header_bytes, ev_type=h.ev_type, ev_size=h.ev_size,
                header_lines=h.header_lines)


def decode(records):
    """decode_event over 8-byte records (bytes / uint8 / RECORD_DTYPE) -> EVENT_DTYPE_PPH array (t, x, y, p)."""
    r = np.frombuffer(bytes(records), np.uint8) if not isinstance(records, np.ndarray) else \
        np.ascontiguousarray(records).view(np.uint8).reshape(-1)
    n = r.size // 8
    out = np.zeros(n, EVENT_DTYPE_PPH)
    if n:
        load().adder_prophesee_decode(r.ctypes.data, n, out.ctypes.data)
    return out


def scan_groups(records, group_start_t=2, running_t=2):
    """consume()'s group scan -> (records that complete groups, groups, group_start_t, running_t)."""
    r = np.ascontiguousarray(records, RECORD_DTYPE) if isinstance(records, np.ndarray) and records.dtype == RECORD_DTYPE \
        else np.frombuffer(bytes(records), RECORD_DTYPE)
    s, rt, g = C.c_uint32(group_start_t), C.c_uint32(running_t), C.c_uint64(0)
    done = load().adder_prophesee_scan_groups(r.ctypes.data if len(r) else None, len(r), C.byref(s), C.byref(rt),
                                              C.byref(g))
    return done, g.value, s.value, rt.value


def records(t, x, y, p):
    """Builds .dat records from columns (x keeps whatever bits it is given: the decoder masks 10)."""
    t, x, y, p = (np.asarray(v, np.int64) for v in (t, x, y, p))
    r = np.zeros(len(t), RECORD_DTYPE)
    r["t"] = (t & 0xFFFFFFFF).astype(np.uint32)
    r["data"] = ((p << 28) | (y << 14) | x).astype(np.uint32).view(np.int32)
    return r


class HipProphesee(N.SourceHandle):
    """Prophesee::new(ref_time, ..)[.crf(c)] on one device: start() runs the two start-up frames, push() any split
    of the record stream, finish() the end of input.  After a refused push, .bad_index is the stream index of the
    record outside the plane (else None)."""
    PREFIX, DESTROY = "adder_prophesee", "adder_prophesee_destroy"

    def __init__(self, width, height, ref_time=1, crf=NO_CRF, device_id=0):
        self.L = load()
        p = AdderPropheseeParams(abi_version=ABI_VERSION, width=width, height=height, ref_time=ref_time,
                                 crf=NO_CRF if crf is None else crf, device_id=device_id)
        h = C.c_void_p()
        rc = self.L.adder_prophesee_create(C.byref(p), C.byref(h))
        if rc != N.OK:
            raise N.AdderHipError(rc, (self.L.adder_prophesee_last_error(None) or b"").decode())
        self.h, self.params = h, p
        self.width, self.height, self.ref_time, self.device_id = width, height, ref_time, device_id
        self.events_per_step = self.L.adder_prophesee_events_per_step(h)
        self.bad_index = None

    def state(self):
        rt, gs, op, pushed = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.adder_prophesee_state(self.h, C.byref(rt), C.byref(gs), C.byref(op), C.byref(pushed)))
        return dict(running_t=rt.value, group_start_t=gs.value, open_records=op.value, records_pushed=pushed.value)

    def start(self):
        need = C.c_uint64(0)
        self.L.adder_prophesee_start(self.h, None, 0, C.byref(need))
        out = np.zeros(max(need.value, 1), N.EVENT_DTYPE)
        n = C.c_uint64(0)
        self._check(self.L.adder_prophesee_start(self.h, out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    def push(self, recs, out_cap=None, stream=None, d_out=None):
        """records: numpy / bytes (host form) or a uint8 CUDA tensor (device form; then the events come back as a
        uint8 CUDA tensor, written into d_out when it is given).  out_cap: events of room (default: the bound of
        2 steps per record, open group included), never more than d_out holds; a push that may not fit raises
        E_OUT_CAPACITY (.needed: a room that succeeds) and changes nothing.  Device tensors must be contiguous and on
        the context's device."""
        self.bad_index = None
        n_out, bad = C.c_uint64(0), C.c_uint64(0)
        if isinstance(recs, (bytes, bytearray, memoryview, np.ndarray)):
            r = np.frombuffer(bytes(recs), np.uint8) if not isinstance(recs, np.ndarray) else \
                np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
            n = r.size // 8
            if out_cap is None:
                out_cap = 2 * (n + self.state()["open_records"]) * self.events_per_step
            out = np.zeros(max(out_cap, 1), N.EVENT_DTYPE)
            rc = self.L.adder_prophesee_push_host(self.h, r.ctypes.data if n else None, n, out.ctypes.data, out_cap,
                                                  C.byref(n_out), C.byref(bad))
            self._done(rc, bad, n_out)
            return out[: n_out.value].copy()
        import torch
        dev = torch.device(f"cuda:{self.device_id}")
        N.device_buffer(recs, dev, "records")
        n = recs.numel() * recs.element_size() // 8
        if out_cap is None:
            out_cap = 2 * (n + self.state()["open_records"]) * self.events_per_step
        d_out, out_cap = self._device_out(dev, out_cap, d_out)
        rc = self.L.adder_prophesee_push_device(self.h, recs.data_ptr() if n else None, n, d_out.data_ptr(), out_cap,
                                                C.byref(n_out), C.byref(bad), C.c_void_p(stream) if stream else None)
        self._done(rc, bad, n_out)
        return d_out[: n_out.value * 12]

    def pixel_state(self):
        """The camera state the last accepted push left -> (last t, last ln): (H, W) uint32 and float64 planes."""
        t = np.zeros((self.height, self.width), np.uint32)
        ln = np.zeros((self.height, self.width), np.float64)
        self._check(self.L.adder_prophesee_pixel_state(self.h, t.ctypes.data, ln.ctypes.data))
        return t, ln


def stream_meta(width, height, ref_time, compressed):
    """The output stream's metadata as the tool writes it: Dvs, AbsoluteT, tps = ref_time * 10^6 (u32),
    delta_t_max = 2 * ref_time; the compressed stream's adu_interval = (tps as f32 / ref_time as f32) as usize."""
    tps = (ref_time * SOURCE_TPS) & 0xFFFFFFFF
    adu = int(np.float32(tps) / np.float32(ref_time)) if compressed else 0
    return dict(width=width, height=height, tps=tps, ref_interval=ref_time, delta_t_max=(2 * ref_time) & 0xFFFFFFFF,
                source_camera=SOURCE_CAMERA_DVS, adu_interval=adu)


def prophesee_to_adder_file(dat, out, ref_time=1, crf=3, compressed=True, chunk_records=1 << 22, device_id=0):
    """prophesee_to_adder: a Prophesee .dat file -> an ADDER file, compressed (the tool's only format) or raw.
    The records are streamed through the device in chunks; the start-up frames, every complete group and
    end_events are written.  crf: 0..9 or None (no crf call).  --delta-t-max is not used by the reference and is not
    taken; feature detection is not built.  -> dict(width, height, records, events)."""
    from .video import raw_header, raw_events, raw_eof
    size = os.path.getsize(dat)
    with open(dat, "rb") as f:
        head = f.read(1 << 16)
        while True:
            try:
                hdr = parse_header(head, size)
                break
            except N.AdderHipError as e:
                if e.code != N.E_OUT_CAPACITY:
                    raise
                more = f.read(len(head))
                head += more
        W, H = hdr["width"], hdr["height"]
        meta = stream_meta(W, H, ref_time, compressed)
        pr = HipProphesee(W, H, ref_time, NO_CRF if crf is None else crf, device_id)
        enc = None
        with open(out, "wb") as g:
            if compressed:
                from .compressed import CompressedEncoder
                q = DEFAULT_CRF_QUALITY if crf is None else crf
                enc = CompressedEncoder(W, H, 1, tps=meta["tps"], ref_interval=ref_time, delta_t_max=meta["delta_t_max"],
                                        adu_interval=meta["adu_interval"], codec_version=CODEC_VERSION,
                                        source_camera=SOURCE_CAMERA_DVS, time_mode=N.TIME_ABSOLUTE_T,
                                        c_thresh_max=CRF[q][1])
                sink = enc.ingest
            else:
                g.write(raw_header(CODEC_VERSION, W, H, 1, meta["tps"], ref_time, meta["delta_t_max"],
                                   source_camera=SOURCE_CAMERA_DVS, time_mode=N.TIME_ABSOLUTE_T))

                def sink(ev):
                    g.write(raw_events(ev, 1))
            n_events = 0
            for ev in [pr.start()]:
                sink(ev)
                n_events += len(ev)
            f.seek(hdr["header_bytes"])
            n_rec = 0
            while True:
                buf = f.read(chunk_records * 8)
                n = len(buf) // 8
                if n == 0:
                    break
                ev = pr.push(buf[: n * 8])
                sink(ev)
                n_events += len(ev)
                n_rec += n
                if len(buf) < chunk_records * 8:
                    break
            ev = pr.finish()
            sink(ev)
            n_events += len(ev)
            if compressed:
                g.write(enc.close())
                enc.destroy()
            else:
                g.write(raw_eof())
        pr.close()
    return dict(width=W, height=H, records=n_rec, events=n_events)
