"""The compressed codec's source model on the device -- HipCompressedModel binds include/adder_compressed_model.h
(DESIGN 5s).  Events in HBM -> per finished ADU the range coder's symbol words (for CompressedEncoder.ingest_symbols)
and the decoder-exact reconstructed events (what compressed_decode would return), both left in HBM.
compress_events_device chains the model and the host coder.  Nothing is computed here."""
import ctypes as C

import numpy as np

from . import _native as N
from .compressed import CompressedEncoder

# the symbol word (csrc/adder_compressed_logic.hpp): context << 10 | fenwick index
CTX_D, CTX_T, CTX_BITSHIFT, CTX_EOF = 0, 1, 2, 3
SYMBOL_INDEX_BITS = 10
SYMBOL_EOF = CTX_EOF << SYMBOL_INDEX_BITS
SYMBOL_NO_EVENT = 256 + 255 + 1
SYMBOL_SKIP_CUBE = 257 + 255 + 1


class AdderCompressedModelCounters(C.Structure):
    _fields_ = [("events_in", C.c_uint64), ("events_dropped", C.c_uint64), ("bitshift", C.c_uint64 * 16)]


_vp, _i32, _u32, _u64, _sz = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_size_t
SYMBOLS = {
    "adder_compressed_model_create": (_i32, [C.POINTER(N.AdderCompressedParams), _i32, C.POINTER(_vp)]),
    "adder_compressed_model_destroy": (None, [_vp]),
    "adder_compressed_model_last_error": (C.c_char_p, [_vp]),
    "adder_compressed_model_set_symbol_capacity": (_i32, [_vp, _u64]),
    "adder_compressed_model_needed": (_i32, [_vp, C.POINTER(_u64)]),
    "adder_compressed_model_ingest_device": (_i32, [_vp, _vp, _sz, _vp]),
    "adder_compressed_model_close": (_i32, [_vp]),
    "adder_compressed_model_adus": (_i32, [_vp, C.POINTER(_u32)]),
    "adder_compressed_model_adu_info": (_i32, [_vp, _u32, _vp, _vp, _vp]),
    "adder_compressed_model_symbols_device": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    "adder_compressed_model_symbols": (_i32, [_vp, _vp, _u64]),
    "adder_compressed_model_events_device": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_u64)]),
    "adder_compressed_model_events": (_i32, [_vp, _vp, _u64]),
    "adder_compressed_model_counters": (_i32, [_vp, C.POINTER(AdderCompressedModelCounters)]),
    "adder_compressed_model_open_adu": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u32)]),
    "adder_compressed_model_last_device_ms": (_i32, [_vp, C.POINTER(C.c_float)]),
}


def load():
    return N.bind(SYMBOLS)


class HipCompressedModel(N.Handle):
    """ingest(events) / finish() model every ADU the call finishes; the call's results are then in .adus,
    .start_t, .symbol_offsets, .event_offsets (numpy), symbols() / events() (CUDA tensors, copies) and
    symbols_host() / events_host() (numpy).  symbol_capacity: None lets the symbol buffer grow; a number makes a call
    that needs more raise E_OUT_CAPACITY with .needed and change nothing, so that it can be made again."""

    DESTROY = "adder_compressed_model_destroy"

    def __init__(self, width, height, channels=1, *, ref_interval, adu_interval, delta_t_max=None, c_thresh_max=7,
                 tps=0, device_id=0, symbol_capacity=None):
        self.L = load()
        p = N.AdderCompressedParams()
        self.L.adder_compressed_default_params(C.byref(p), width, height, channels)
        p.ref_interval, p.adu_interval, p.c_thresh_max = ref_interval, adu_interval, c_thresh_max
        p.delta_t_max = delta_t_max if delta_t_max is not None else ref_interval * adu_interval
        p.tps = tps or p.tps
        h = C.c_void_p()
        rc = self.L.adder_compressed_model_create(C.byref(p), device_id, C.byref(h))
        if rc != N.OK:
            raise N.AdderHipError(rc, (self.L.adder_compressed_model_last_error(None) or b"").decode())
        self.h, self.params, self.device_id = h, p, device_id
        self.width, self.height, self.channels = width, height, channels
        self._results(0)
        if symbol_capacity is not None:
            self.set_symbol_capacity(symbol_capacity)

    def _error(self, rc):
        err = N.AdderHipError(rc, (self.L.adder_compressed_model_last_error(self.h) or b"").decode())
        n = C.c_uint64(0)
        self.L.adder_compressed_model_needed(self.h, C.byref(n))
        err.needed = n.value
        return err

    def _check(self, rc):
        if rc != N.OK:
            self._results(0)
            raise self._error(rc)

    def _results(self, k):
        self.adus = k
        self.start_t = np.zeros(k, np.uint32)
        self.symbol_offsets = np.zeros(k + 1, np.uint64)
        self.event_offsets = np.zeros(k + 1, np.uint64)
        if k:
            self._check(self.L.adder_compressed_model_adu_info(self.h, k, self.start_t.ctypes.data,
                                                               self.symbol_offsets.ctypes.data,
                                                               self.event_offsets.ctypes.data))

    def _after(self, rc):
        self._check(rc)
        k = C.c_uint32(0)
        self._check(self.L.adder_compressed_model_adus(self.h, C.byref(k)))
        self._results(k.value)
        return k.value

    def set_symbol_capacity(self, words):
        """None or 0: the buffer grows with the calls."""
        self._check(self.L.adder_compressed_model_set_symbol_capacity(self.h, int(words or 0)))

    def ingest(self, events, stream=None):
        """events: AdderEvents in stream order -- a CUDA tensor (uint8, 12 bytes an event, or any dtype of whole
        events) or a numpy array of EVENT_DTYPE, which is uploaded.  -> the ADUs the call finished."""
        import torch
        if isinstance(events, torch.Tensor):
            t = events
        else:
            a = np.ascontiguousarray(events, dtype=N.EVENT_DTYPE)
            t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(f"cuda:{self.device_id}")
        N.device_buffer(t, torch.device("cuda", self.device_id), "events")
        nbytes = t.numel() * t.element_size()
        if nbytes % 12:
            raise ValueError("events: not a whole number of 12-byte AdderEvents")
        s = getattr(stream, "cuda_stream", stream)
        if s is None:
            s = torch.cuda.current_stream(t.device).cuda_stream
        rc = self.L.adder_compressed_model_ingest_device(self.h, t.data_ptr() if nbytes else None, nbytes // 12,
                                                         C.c_void_p(s) if s else None)
        return self._after(rc)

    def finish(self):
        """adder_compressed_model_close: models the partial last ADU (if it holds an event); no events after it.
        -> the ADUs finished: 0 or 1.  (close(), as of every handle here, frees the object.)"""
        return self._after(self.L.adder_compressed_model_close(self.h))

    def device_ms(self):
        """The device's share of the last ingest / finish: the sum of the spans between the call's host waits (copies,
        kernels, sort and scans), by events on its stream."""
        ms = C.c_float(0.0)
        self._check(self.L.adder_compressed_model_last_device_ms(self.h, C.byref(ms)))
        return ms.value

    def symbols(self):
        """The call's symbol words: a CUDA tensor of dtype int16 (the words' bit patterns), a copy."""
        import torch
        n = int(self.symbol_offsets[-1])
        out = torch.empty(n, dtype=torch.int16, device=f"cuda:{self.device_id}")
        self._check(self.L.adder_compressed_model_symbols(self.h, out.data_ptr() if n else None, n))
        return out

    def events(self):
        """The call's reconstructed events: a uint8 CUDA tensor of 12 bytes an event, a copy."""
        import torch
        n = int(self.event_offsets[-1])
        out = torch.empty(12 * n, dtype=torch.uint8, device=f"cuda:{self.device_id}")
        self._check(self.L.adder_compressed_model_events(self.h, out.data_ptr() if n else None, n))
        return out

    def symbols_host(self):
        out = np.zeros(int(self.symbol_offsets[-1]), np.uint16)
        self._check(self.L.adder_compressed_model_symbols(self.h, out.ctypes.data, len(out)))
        return out

    def events_host(self):
        out = np.zeros(int(self.event_offsets[-1]), N.EVENT_DTYPE)
        self._check(self.L.adder_compressed_model_events(self.h, out.ctypes.data, len(out)))
        return out

    def counters(self):
        c = AdderCompressedModelCounters()
        self._check(self.L.adder_compressed_model_counters(self.h, C.byref(c)))
        return {"events_in": c.events_in, "events_dropped": c.events_dropped, "bitshift": [int(v) for v in c.bitshift]}

    def open_adu(self):
        """-> (events of the still-open ADU, its start_t)"""
        n, t = C.c_uint64(0), C.c_uint32(0)
        self._check(self.L.adder_compressed_model_open_adu(self.h, C.byref(n), C.byref(t)))
        return n.value, t.value


def compress_events_device(events, width, height, channels=1, *, tps, ref_interval, delta_t_max, adu_interval,
                           c_thresh_max=7, codec_version=3, source_camera=0, time_mode=N.TIME_ABSOLUTE_T,
                           write_header=True, threads=0, device_id=0, pieces=1):
    """events (a CUDA tensor or numpy, stream order) -> (stream_bytes, recon_events): the compressed stream the host
    sink writes for them -- the model on the device, the range coder on the host -- and the events a decoder gets back
    from it (a uint8 CUDA tensor, 12 bytes an event).  pieces: the calls the events are cut into."""
    import torch
    model = HipCompressedModel(width, height, channels, ref_interval=ref_interval, adu_interval=adu_interval,
                               delta_t_max=delta_t_max, c_thresh_max=c_thresh_max, tps=tps, device_id=device_id)
    enc = CompressedEncoder(width, height, channels, tps=tps, ref_interval=ref_interval, delta_t_max=delta_t_max,
                            adu_interval=adu_interval, codec_version=codec_version, source_camera=source_camera,
                            time_mode=time_mode, c_thresh_max=c_thresh_max, write_header=write_header, threads=threads)
    try:
        if not isinstance(events, torch.Tensor):
            a = np.ascontiguousarray(events, dtype=N.EVENT_DTYPE)
            events = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(f"cuda:{device_id}")
        flat = events.reshape(-1).view(torch.uint8)
        n = flat.numel() // 12
        recon = []

        def hand_over():
            if not model.adus:
                return
            sym = model.symbols_host()
            for a in range(model.adus):
                enc.ingest_symbols(sym[int(model.symbol_offsets[a]): int(model.symbol_offsets[a + 1])])
            recon.append(model.events())

        step = max(1, -(-n // max(1, pieces)))
        for lo in range(0, n, step):
            model.ingest(flat[12 * lo: 12 * min(n, lo + step)])
            hand_over()
        model.finish()
        hand_over()
        out = enc.close()
        rec = torch.cat(recon) if recon else torch.empty(0, dtype=torch.uint8, device=f"cuda:{device_id}")
        return out, rec
    finally:
        enc.destroy()
        model.close()
