"""Shared by test_color_cpu.py and test_gpu_color.py: the reference form of the colour-to-gray step (utils/cv.rs:215-232)
in numpy, the frame of all 2^24 triples, and the shapes of the edge cases."""
import functools

import numpy as np


def gray_reference(rgb):
    """(ch0 as f64 * 0.114 + ch1 as f64 * 0.587 + ch2 as f64 * 0.299) as u8 -- separate multiplies and adds in float64,
    left to right; the sum never leaves [0, 255], so astype(uint8) is Rust's truncating `as u8`.  rgb: [..., 3] u8."""
    rgb = np.asarray(rgb)
    p0 = rgb[..., 0].astype(np.float64) * 0.114
    p1 = rgb[..., 1].astype(np.float64) * 0.587
    p2 = rgb[..., 2].astype(np.float64) * 0.299
    s = p0 + p1
    s = s + p2
    assert s.size == 0 or (s.min() >= 0.0 and s.max() <= 255.0)
    return s.astype(np.uint8)


def gray_integer(rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    return ((114 * rgb[..., 0] + 587 * rgb[..., 1] + 299 * rgb[..., 2]) // 1000).astype(np.uint8)


def gray_float32(rgb):
    rgb = np.asarray(rgb)
    f = np.float32
    s = rgb[..., 0].astype(f) * f(0.114) + rgb[..., 1].astype(f) * f(0.587)
    s = s + rgb[..., 2].astype(f) * f(0.299)
    return s.astype(np.uint8)


def all_triples():
    """[4096][4096][3] u8: pixel i (row-major) is the triple (i >> 16, (i >> 8) & 255, i & 255)."""
    i = np.arange(1 << 24, dtype=np.uint32)
    out = np.empty((1 << 24, 3), np.uint8)
    out[:, 0] = i >> 16
    out[:, 1] = (i >> 8) & 255
    out[:, 2] = i & 255
    return out.reshape(4096, 4096, 3)


@functools.lru_cache(maxsize=1)
def all_triples_gray():
    """gray_reference of all_triples(), [4096][4096] u8 (computed once per process, in slabs; read-only)."""
    rgb = all_triples()
    out = np.empty((4096, 4096), np.uint8)
    for r in range(0, 4096, 256):
        out[r:r + 256] = gray_reference(rgb[r:r + 256])
    out.setflags(write=False)
    return out


# widths around the dword path's edges (a lane converts four pixels; a block is 64 lanes wide) and an odd large one
EDGE_WIDTHS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 257, 1021)
GUARD = 0xA5
