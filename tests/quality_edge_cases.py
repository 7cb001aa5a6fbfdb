"""Shapes and contents of the quality kernels' edge tests (tests/test_gpu_quality_edges.py), shared with the CPU checks
of tests/test_quality_cpu.py.  The shapes follow the constants of csrc/adder_quality_kernels.h (kernel_constants)."""
import numpy as np

import kernel_constants

EXTREMES = ("all-255 both", "255 against 0", "checkerboard against its inverse", "constant against noise")
GRID_ROWS_MAX = 65535  # rows of a HIP grid: quality_group_frames puts 65535 / channels frames into a launch group


def tile_edge_widths(k=None):
    """Plane widths whose windows per row sit on the edges of the SSIM tile: one window, a tile less one / full / plus
    one window column, a last tile of 7 and of 8 windows, two full tiles, and one more."""
    tw = (k or kernel_constants.quality())["kSsimTileW"]
    return [ww + 7 for ww in (1, 2, 8, tw - 1, tw, tw + 1, tw + 7, tw + 8, 2 * tw, 2 * tw + 1)]


def tile_edge_heights(k=None):
    """Plane heights whose window rows sit on the edges of the tile and of the row loop's unrolled eight steps: a tile
    with one row, rows around 8, around a full tile and two; 2 .. 6 add the phases of the loop that those leave out."""
    th = (k or kernel_constants.quality())["kSsimTileH"]
    return [wh + 7 for wh in (1, 2, 3, 4, 5, 6, 7, 8, 9, th - 1, th, th + 1, 2 * th, 2 * th + 1)]


def unlike_channels(rng, n, H, W, C):
    """Random frames [n][H][W][C].  C = 3: one channel identical in both inputs, one inverted, one independent noise,
    the roles moving on by one from frame to frame, so a mixed-up channel or frame shows.  C = 1: frame by frame
    a near copy (+-3) and independent noise in turn."""
    a = rng.integers(0, 256, (n, H, W, C), dtype=np.uint8)
    b = np.empty_like(a)
    for f in range(n):
        for ch in range(C):
            role = (f + ch) % 3 if C == 3 else 2 + (f + 1) % 2
            if role == 0:
                b[f, ..., ch] = a[f, ..., ch]
            elif role == 1:
                b[f, ..., ch] = 255 - a[f, ..., ch]
            elif role == 2:
                b[f, ..., ch] = rng.integers(0, 256, (H, W), dtype=np.uint8)
            else:
                b[f, ..., ch] = np.clip(a[f, ..., ch].astype(np.int16) + rng.integers(-3, 4, (H, W)), 0, 255)
    return a, b


def extreme_pair(kind, rng, H, W, C):
    """One frame pair [H][W][C] of EXTREMES[kind]: the contents at which the kernel's packed 16-bit halves and its
    32-bit integer expressions reach their maxima, and (checkerboard) its most negative windows."""
    if kind == 0:
        return np.full((H, W, C), 255, np.uint8), np.full((H, W, C), 255, np.uint8)
    if kind == 1:
        return np.full((H, W, C), 255, np.uint8), np.zeros((H, W, C), np.uint8)
    if kind == 2:
        y, x = np.mgrid[0:H, 0:W]
        board = (((x + y) & 1) * 255).astype(np.uint8)
        a = np.repeat(board[:, :, None], C, axis=2)
        return a, 255 - a
    return np.full((H, W, C), 200, np.uint8), rng.integers(0, 256, (H, W, C), dtype=np.uint8)


def extreme_frames(rng, kinds, H, W, C):
    """The pairs of `kinds` stacked into two batches [len(kinds)][H][W][C]."""
    pairs = [extreme_pair(k, rng, H, W, C) for k in kinds]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def sse_clamp_plane(k=None):
    """(W, H) of the one-channel plane just past the bytes at which quality_shape clamps the SSE grid; a multiple of
    16 bytes, so the 16-byte path takes it."""
    k = k or kernel_constants.quality()
    clamp = k["kSseMaxBlocks"] * k["kSseBytesPerBlock"]
    W = 8192
    assert clamp % W == 0
    return W, clamp // W + 1, clamp


def known_changes(rng, a, clamp):
    """-> (b, sse): b is the flat uint8 array a with about 1000 bytes changed by known amounts -- byte 0, the last
    byte, both sides of 16-byte boundaries, bytes around and past offset `clamp`, random ones -- and sse the sum of
    the squared changes."""
    n = a.size
    pos = [0, n - 1, n - 16, n - 17]
    for edge in (16, 32, 4096, clamp // 2, clamp - 16, clamp, clamp + 16, clamp + 4096):
        pos += [edge - 1, edge, edge + 15, edge + 16]
    pos += rng.integers(0, n, 900).tolist() + rng.integers(clamp, n, 60).tolist()
    pos = np.unique(np.array(pos, np.int64))
    assert pos[0] == 0 and pos[-1] == n - 1 and (pos > clamp).sum() >= 60
    d = rng.integers(1, 128, len(pos))
    v = a[pos].astype(np.int64)
    b = a.copy()
    b[pos] = np.where(v + d <= 255, v + d, v - d).astype(np.uint8)
    return b, int((d * d).sum())
