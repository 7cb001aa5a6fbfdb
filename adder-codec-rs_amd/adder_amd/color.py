"""Colour frames to gray as a one-channel transcode of the reference sees them (include/adder_color.h): Framed::consume
(framed.rs:127-134) runs every decoded three-channel frame through utils/cv.rs:215-232,

    gray = (ch0 as f64 * 0.114 + ch1 as f64 * 0.587 + ch2 as f64 * 0.299) as u8

in f64, left to right, nothing fused.  to_gray_device is the HIP kernel on torch tensors, to_gray_host the library's CPU
loop over the same per-pixel function (it needs no device); both give the reference's byte for all 2^24 triples
(DESIGN 5o).  HipVideo's *_rgb methods feed colour frames straight into a one-channel context."""
import ctypes as C

import numpy as np

from . import _native as N

_vp, _i32, _u32, _sz = C.c_void_p, C.c_int, C.c_uint32, C.c_size_t
SYMBOLS = {
    "adder_color_to_gray_device": (_i32, [_vp, _sz, _sz, _vp, _sz, _sz, _u32, _u32, _u32, _vp]),
    "adder_color_to_gray_host": (_i32, [_vp, _sz, _sz, _vp, _sz, _sz, _u32, _u32, _u32]),
    "adder_color_last_error": (C.c_char_p, []),
}


def load():
    return N.bind(SYMBOLS)


def _check(L, rc):
    if rc != N.OK:
        raise N.AdderHipError(rc, (L.adder_color_last_error() or b"").decode())


def _frames_view(a, last):
    """(frames, rows, width, [last]) of an array / tensor of 2 + (last > 1) .. 3 + (last > 1) dimensions."""
    shape = tuple(a.shape)
    if last > 1:
        if len(shape) < 3 or shape[-1] != last:
            raise ValueError(f"expected [..., rows, width, {last}], got {shape}")
        shape = shape[:-1]
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3:
        raise ValueError(f"expected [frames,] rows, width{', 3' if last > 1 else ''}; got {tuple(a.shape)}")
    return shape


def _byte_strides(strides, shape, what):
    """(row, frame) byte strides of a [frames][rows][width](x3) view whose pixels are contiguous; a dimension of one
    element has no stride to speak of: 0 (packed)."""
    frames, rows, _ = shape
    row = strides[-2] if rows > 1 else 0
    frame = strides[-3] if len(strides) >= 3 and frames > 1 else 0
    if row < 0 or frame < 0:
        raise ValueError(f"{what}: negative strides")
    return int(row), int(frame)


def to_gray_device(d_rgb, d_gray=None, stream=None):
    """d_rgb: uint8 CUDA tensor [frames,] rows, width, 3 -- any view whose pixels are contiguous (stride 3 and 1 in the
    last two dimensions); row and frame strides are taken from the tensor.  d_gray: uint8 CUDA tensor [frames,] rows,
    width with contiguous rows (None: a new packed one).  One launch, asynchronous on `stream` (a torch.cuda.Stream or
    its handle; None: the default stream).  Returns d_gray."""
    import torch
    L = load()
    shape = _frames_view(d_rgb, 3)
    if d_gray is None:
        d_gray = torch.empty(tuple(d_rgb.shape[:-1]), dtype=torch.uint8, device=d_rgb.device)
    if _frames_view(d_gray, 1) != shape:
        raise ValueError(f"d_gray {tuple(d_gray.shape)} does not match d_rgb {tuple(d_rgb.shape)}")
    for t in (d_rgb, d_gray):
        if not (t.is_cuda and t.dtype == torch.uint8):
            raise ValueError("to_gray_device takes uint8 CUDA tensors")
    wide = shape[2] > 1  # (a dimension of one element may carry any stride)
    if d_rgb.stride(-1) != 1 or (wide and (d_rgb.stride(-2) != 3 or d_gray.stride(-1) != 1)):
        raise ValueError("the pixels of a row must be contiguous")
    ss = _byte_strides(d_rgb.stride()[:-1], shape, "d_rgb")
    ds = _byte_strides(d_gray.stride(), shape, "d_gray")
    s = getattr(stream, "cuda_stream", stream)
    _check(L, L.adder_color_to_gray_device(d_rgb.data_ptr(), ss[0], ss[1], d_gray.data_ptr(), ds[0], ds[1], shape[2], shape[1],
                                           shape[0], C.c_void_p(s) if s else None))
    return d_gray


def to_gray_host(rgb):
    """rgb: uint8 array [frames,] rows, width, 3 (strided views are passed as they are) -> a new packed uint8 array
    [frames,] rows, width.  Runs on the CPU."""
    L = load()
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8:
        raise ValueError("to_gray_host takes uint8 frames")
    shape = _frames_view(rgb, 3)
    if rgb.strides[-1] != 1 or (shape[2] > 1 and rgb.strides[-2] != 3) or any(s < 0 for s in rgb.strides):
        rgb = np.ascontiguousarray(rgb)
    out = np.empty(rgb.shape[:-1], np.uint8)
    ss = _byte_strides(rgb.strides[:-1], shape, "rgb")
    _check(L, L.adder_color_to_gray_host(rgb.ctypes.data, ss[0], ss[1], out.ctypes.data, 0, 0, shape[2], shape[1], shape[0]))
    return out
