"""Dense FAST 9_16 over whole frames and the feature precision / recall / accuracy -- HipFastEval binds
include/adder_fast.h.  The reference's feature log (video.rs:926-1060) runs the frame-based detector over
the running-intensities plane after every frame and scores the event-driven features against it
(utils/cv.rs:235-279); both inputs live in HBM here: HipVideo.running_intensities_device and
HipVideo.feature_set_device."""
import ctypes as C

import numpy as np

from . import _native as N

# include/adder_fast.h
ABI_VERSION = 1
DEFAULT_THRESHOLD = 30


class AdderFastParams(C.Structure):
    """include/adder_fast.h::AdderFastParams"""
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("width", C.c_uint16),
        ("height", C.c_uint16),
        ("channels", C.c_uint8),
        ("threshold", C.c_uint8),
        ("nonmax", C.c_uint8),
        ("reserved0", C.c_uint8),
        ("device_id", C.c_int32),
    ]


class AdderFastEval(C.Structure):
    _fields_ = [("tp", C.c_uint64), ("fp", C.c_uint64), ("tn", C.c_uint64), ("fn", C.c_uint64),
                ("gt_count", C.c_uint64), ("pred_count", C.c_uint64),
                ("precision", C.c_double), ("recall", C.c_double), ("accuracy", C.c_double)]


_vp, _i32, _u32, _u64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
SYMBOLS = {
    "adder_fast_create": (_i32, [C.POINTER(AdderFastParams), C.POINTER(_vp)]),
    "adder_fast_destroy": (None, [_vp]),
    "adder_fast_last_error": (C.c_char_p, [_vp]),
    "adder_fast_detect_device": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _u64, _vp, _vp]),
    "adder_fast_detect_host": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _u64, _vp]),
    "adder_fast_mask_from_xy_device": (_i32, [_vp, _vp, _u64, _vp, _vp]),
    "adder_fast_evaluate_device": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "adder_fast_evaluate_host": (_i32, [_vp, _vp, _vp, _u32, _vp]),
}
EVAL_KEYS = ("tp", "fp", "tn", "fn", "gt_count", "pred_count", "precision", "recall", "accuracy")


def load():
    return N.bind(SYMBOLS)


def _ptr(t):
    return t.data_ptr() if t is not None else None


class HipFastEval(N.Handle):
    """Dense FAST over u8 frames [n][H][W][C] (C = 1 or 3, channel 0 examined) on the device, and the score of a
    predicted feature set against it.

    threshold 1..255 (30: the event detectors' INTENSITY_THRESHOLD); nonmax: keep a corner only where its score is
    strictly above its 8 neighbours'.  A call's errors carry the library's code (.code), E_OUT_CAPACITY with .counts."""

    DESTROY = "adder_fast_destroy"

    def __init__(self, width, height, channels=1, *, threshold=DEFAULT_THRESHOLD, nonmax=False, device_id=0):
        self.N, self.L = N, load()
        if not 0 <= int(threshold) <= 255:
            raise ValueError("threshold: 1 .. 255")
        p = AdderFastParams(abi_version=ABI_VERSION, width=width, height=height, channels=channels,
                            threshold=int(threshold), nonmax=1 if nonmax else 0, device_id=device_id)
        h = C.c_void_p()
        rc = self.L.adder_fast_create(C.byref(p), C.byref(h))
        if rc != N.OK:
            raise N.AdderHipError(rc, (self.L.adder_fast_last_error(None) or b"").decode())
        self.h, self.params = h, p
        self.width, self.height, self.channels = width, height, channels
        self.threshold, self.nonmax, self.device_id = int(threshold), bool(nonmax), device_id
        self.plane = width * height
        self.frame_elems = self.plane * channels

    def _error(self, rc):
        return self.N.AdderHipError(rc, (self.L.adder_fast_last_error(self.h) or b"").decode())

    def _n_frames(self, frames):
        size = frames.numel() if hasattr(frames, "numel") else frames.size
        n, rem = divmod(size, self.frame_elems)
        if rem:
            raise ValueError(f"{tuple(frames.shape)} is not a whole number of {self.height}x{self.width}x{self.channels} frames")
        return n

    def _dev(self, t, what, elems, itemsize=1):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.element_size() == itemsize
                and t.numel() >= elems):
            raise ValueError(f"{what}: a contiguous CUDA tensor of >= {elems} elements of {itemsize} byte(s) is needed")

    @staticmethod
    def _stream(stream):
        s = getattr(stream, "cuda_stream", stream)
        return C.c_void_p(s) if s else None

    def _dicts(self, res, n):
        return [{k: getattr(res[i], k) for k in EVAL_KEYS} for i in range(n)]

    def detect_device(self, frames, mask=None, score=None, xy=None, stream=None):
        """frames: a contiguous uint8 CUDA tensor of n whole frames.  mask / score: uint8 CUDA tensors of n * H * W
        elements, written in place; xy: a uint32 (or int32) CUDA tensor whose length is the capacity of the coordinate
        list (x | y << 16, raster order, frame after frame).  Each may be None.  Queued on `stream` (a
        torch.cuda.Stream or its handle; None: the default stream); waits for its own results.  -> counts, int64 [n]."""
        n = self._n_frames(frames)
        self._dev(frames, "frames", n * self.frame_elems)
        if mask is not None:
            self._dev(mask, "mask", n * self.plane)
        if score is not None:
            self._dev(score, "score", n * self.plane)
        cap = 0
        if xy is not None:
            self._dev(xy, "xy", 0, 4)
            cap = xy.numel()
        counts = np.zeros(max(n, 1), np.uint64)
        rc = self.L.adder_fast_detect_device(self.h, frames.data_ptr(), n, _ptr(mask), _ptr(score), _ptr(xy), cap,
                                             counts.ctypes.data, self._stream(stream))
        counts = counts[:n].astype(np.int64)
        if rc != N.OK:
            err = self._error(rc)
            err.counts = counts
            raise err
        return counts

    def detect(self, frames, mask=True, score=False, xy=False, capacity=None):
        """The same for a numpy uint8 array of n whole frames (the host-pointer form).  mask / score / xy choose the
        outputs; capacity: the room of the coordinate list (None: every position).
        -> {"counts": int64 [n], "mask": [n][H][W] | None, "score": [n][H][W] | None, "xy": uint32 [total] | None}."""
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        n = self._n_frames(a)
        m = np.zeros((n, self.height, self.width), np.uint8) if mask else None
        s = np.zeros((n, self.height, self.width), np.uint8) if score else None
        cap = n * self.plane if capacity is None else int(capacity)
        c = np.zeros(max(cap, 1), np.uint32) if xy else None
        counts = np.zeros(max(n, 1), np.uint64)
        rc = self.L.adder_fast_detect_host(self.h, a.ctypes.data, n, m.ctypes.data if mask else None,
                                           s.ctypes.data if score else None, c.ctypes.data if xy else None, cap,
                                           counts.ctypes.data)
        counts = counts[:n].astype(np.int64)
        if rc != N.OK:
            err = self._error(rc)
            err.counts, err.mask, err.score = counts, m, s
            raise err
        return {"counts": counts, "mask": m, "score": s, "xy": c[: int(counts.sum())].copy() if xy else None}

    def mask_from_xy(self, xy, mask=None, stream=None):
        """xy: a uint32 (or int32) CUDA tensor of packed coordinates x | y << 16 -> the uint8 CUDA tensor `mask`
        ([H][W]; None: a new one) cleared and set to 1 at each of them.  A coordinate outside the plane raises
        (E_BAD_PARAMS) and leaves the plane as it was."""
        import torch
        self._dev(xy, "xy", 0, 4)
        if mask is None:
            mask = torch.empty((self.height, self.width), dtype=torch.uint8, device=xy.device)
        self._dev(mask, "mask", self.plane)
        rc = self.L.adder_fast_mask_from_xy_device(self.h, xy.data_ptr() if xy.numel() else None, xy.numel(),
                                                   mask.data_ptr(), self._stream(stream))
        if rc != N.OK:
            raise self._error(rc)
        return mask

    def evaluate_device(self, frames, prediction, stream=None):
        """frames: n whole frames; prediction: n * H * W uint8 (nonzero = predicted), both contiguous CUDA tensors.
        -> one dict per frame: tp, fp, tn, fn, gt_count, pred_count, precision, recall, accuracy (NaN for 0 / 0)."""
        n = self._n_frames(frames)
        self._dev(frames, "frames", n * self.frame_elems)
        self._dev(prediction, "prediction", n * self.plane)
        if prediction.numel() != n * self.plane:
            raise ValueError("prediction: one H x W plane per frame")
        res = (AdderFastEval * max(n, 1))()
        rc = self.L.adder_fast_evaluate_device(self.h, frames.data_ptr(), prediction.data_ptr(), n, res,
                                               self._stream(stream))
        if rc != N.OK:
            raise self._error(rc)
        return self._dicts(res, n)

    def evaluate(self, frames, prediction):
        """The same for numpy uint8 arrays (the host-pointer form)."""
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        b = np.ascontiguousarray(prediction, dtype=np.uint8)
        n = self._n_frames(a)
        if b.size != n * self.plane:
            raise ValueError("prediction: one H x W plane per frame")
        res = (AdderFastEval * max(n, 1))()
        rc = self.L.adder_fast_evaluate_host(self.h, a.ctypes.data, b.ctypes.data, n, res)
        if rc != N.OK:
            raise self._error(rc)
        return self._dicts(res, n)
