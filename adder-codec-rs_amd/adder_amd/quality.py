"""Quality metrics of a reconstruction against its source frame -- the host-side mirror of
adder-codec-rs/src/utils/cv.rs:306-360 (`calculate_quality_metrics`: MSE over every element in f64, an MSE of exactly 0
replaced by 1e-7 "so that PSNR isn't undefined", PSNR = 20 log10(255) - 10 log10(MSE)).  The reference applies it to the input
frame against the transcoder's running intensities (framed.rs:136-151, feature "feature-logging") and, in its viewer, against
the framer's reconstruction (adder-viz/src/transcoder/adder.rs:318): the harness of SURVEY 8(f)1 does the latter.  The squared
differences are integers below 2^16 and their sum stays far below 2^53, so the f64 sum is exact in any order: numpy's equals
the reference's sequential loop bit for bit.  SSIM (cv.rs:362-430) is computed on the device only: HipQuality binds
include/adder_quality.h, all three metrics of frame batches in HBM or host memory."""
import ctypes as C
import math

import numpy as np

from . import _native as N


def calculate_mse(original, reconstructed):
    a = np.asarray(original)
    b = np.asarray(reconstructed)
    if a.shape != b.shape:
        raise ValueError("Shapes of original and reconstructed images must match")   # cv.rs:312, :336
    d = a.astype(np.int64) - b.astype(np.int64)
    return float(int((d * d).sum())) / float(a.size)


def calculate_psnr(mse):
    return 20.0 * math.log10(255.0) - 10.0 * math.log10(mse)


def calculate_quality_metrics(original, reconstructed):
    """-> {"mse": .., "psnr": ..} exactly as cv.rs:306-333 fills QualityMetrics {mse: Some, psnr: Some, ssim: None}."""
    mse = calculate_mse(original, reconstructed)
    if mse == 0.0:
        mse = 0.0000001
    return {"mse": mse, "psnr": calculate_psnr(mse)}


# include/adder_quality.h
ABI_VERSION = 1
MSE, PSNR, SSIM = 1, 2, 4


class AdderQualityParams(C.Structure):
    """include/adder_quality.h::AdderQualityParams"""
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("width", C.c_uint16),
        ("height", C.c_uint16),
        ("channels", C.c_uint8),
        ("metrics", C.c_uint8),
        ("reserved0", C.c_uint16),
        ("device_id", C.c_int32),
    ]


class AdderQualityResult(C.Structure):
    _fields_ = [("mse", C.c_double), ("psnr", C.c_double), ("ssim", C.c_double), ("present", C.c_uint32),
                ("reserved", C.c_uint32)]


_vp, _i32, _u32 = C.c_void_p, C.c_int, C.c_uint32
SYMBOLS = {
    "adder_quality_create": (_i32, [C.POINTER(AdderQualityParams), C.POINTER(_vp)]),
    "adder_quality_destroy": (None, [_vp]),
    "adder_quality_last_error": (C.c_char_p, [_vp]),
    "adder_quality_map_elems": (C.c_uint64, [_vp, _u32]),
    "adder_quality_compute_device": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    "adder_quality_compute_host": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp]),
}


def load():
    return N.bind(SYMBOLS)


class HipQuality(N.Handle):
    """calculate_quality_metrics on the device for batches of u8 frames [n][H][W][C] (C = 1 or 3).

    mse / psnr / ssim select the metrics (QualityMetrics' Some / None); every call returns one dict per frame with the
    selected keys.  MSE and PSNR equal calculate_quality_metrics bit for bit; SSIM (percent) is the reference's
    windows bit for bit, summed in a fixed order (NaN when H or W < 8)."""

    DESTROY = "adder_quality_destroy"

    def __init__(self, width, height, channels=1, *, mse=True, psnr=True, ssim=False, device_id=0):
        self.N, self.L = N, load()
        metrics = (MSE if mse else 0) | (PSNR if psnr else 0) | (SSIM if ssim else 0)
        p = AdderQualityParams(abi_version=ABI_VERSION, width=width, height=height, channels=channels,
                               metrics=metrics, device_id=device_id)
        h = C.c_void_p()
        rc = self.L.adder_quality_create(C.byref(p), C.byref(h))
        if rc != N.OK:
            raise N.AdderHipError(rc, (self.L.adder_quality_last_error(None) or b"").decode())
        self.h, self.params = h, p
        self.width, self.height, self.channels, self.metrics = width, height, channels, metrics
        self.frame_elems = width * height * channels

    def map_shape(self, n_frames):
        """The per-window map of n frames: [n][C][H - 7][W - 7] float64 (empty when the plane has no window)."""
        return (n_frames, self.channels, max(self.height - 7, 0), max(self.width - 7, 0))

    def _frames(self, a, b):
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError("Shapes of original and reconstructed images must match")
        n, rem = divmod(a.numel() if hasattr(a, "numel") else a.size, self.frame_elems)
        if rem:
            raise ValueError(f"{tuple(a.shape)} is not a whole number of {self.height}x{self.width}x{self.channels} frames")
        return n

    def _check_map(self, m, n, is_torch):
        need = n * self.channels * max(self.height - 7, 0) * max(self.width - 7, 0)
        if is_torch:
            import torch
            ok = m.dtype == torch.float64 and m.is_cuda and m.is_contiguous() and m.numel() >= need
        else:
            ok = m.dtype == np.float64 and m.flags.c_contiguous and m.size >= need
        if not ok:
            raise ValueError(f"ssim_map must be a contiguous float64 buffer of >= {need} elements")

    def _dicts(self, res, n):
        out = []
        for k in range(n):
            r, d = res[k], {}
            if self.metrics & MSE:
                d["mse"] = r.mse
            if self.metrics & PSNR:
                d["psnr"] = r.psnr
            if self.metrics & SSIM:
                d["ssim"] = r.ssim
            out.append(d)
        return out

    def _check(self, rc):
        if rc != self.N.OK:
            raise self.N.AdderHipError(rc, (self.L.adder_quality_last_error(self.h) or b"").decode())

    def compute_device(self, original, reconstructed, stream=None, ssim_map=None):
        """original / reconstructed: contiguous uint8 CUDA tensors of n whole frames.  Queued on `stream` (a
        torch.cuda.Stream or its handle; None: the default stream) without a host synchronisation in front; waits for
        its own results.  ssim_map: a float64 CUDA tensor of map_shape(n) elements that receives every window's value."""
        n = self._frames(original, reconstructed)
        for t in (original, reconstructed):
            assert t.is_cuda and t.is_contiguous() and t.element_size() == 1
        if ssim_map is not None:
            self._check_map(ssim_map, n, True)
        res = (AdderQualityResult * max(n, 1))()
        s = getattr(stream, "cuda_stream", stream)
        self._check(self.L.adder_quality_compute_device(
            self.h, original.data_ptr(), reconstructed.data_ptr(), n, res,
            ssim_map.data_ptr() if ssim_map is not None else None, C.c_void_p(s) if s else None))
        return self._dicts(res, n)

    def compute(self, original, reconstructed, ssim_map=None):
        """The same for numpy uint8 arrays of n whole frames (the host-pointer form).  ssim_map: a float64 numpy array
        of map_shape(n) elements, written in place."""
        a = np.ascontiguousarray(original, dtype=np.uint8)
        b = np.ascontiguousarray(reconstructed, dtype=np.uint8)
        n = self._frames(a, b)
        if ssim_map is not None:
            self._check_map(ssim_map, n, False)
        res = (AdderQualityResult * max(n, 1))()
        self._check(self.L.adder_quality_compute_host(
            self.h, a.ctypes.data, b.ctypes.data, n, res, ssim_map.ctypes.data if ssim_map is not None else None))
        return self._dicts(res, n)
