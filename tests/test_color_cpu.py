"""The colour-to-gray step (include/adder_color.h) without a GPU: adder_color_to_gray_host over all 2^24 triples against
the reference's expression in numpy float64, the proof that this comparison tells the usual shortcuts apart, strides and
refusals of the host function, and the binding tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adder_amd as A
from adder_amd import color as K

import color_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(src, dst, width, rows, frames, ss=(0, 0), ds=(0, 0), src_off=0, dst_off=0):
    """The raw call on numpy byte buffers -> return code."""
    L = K.load()
    return L.adder_color_to_gray_host(src.ctypes.data + src_off, ss[0], ss[1], dst.ctypes.data + dst_off, ds[0], ds[1], width,
                                      rows, frames)


def test_host_equals_the_reference_on_every_triple():
    rgb = CC.all_triples()
    got = A.to_gray_host(rgb)
    want = CC.all_triples_gray()
    assert got.shape == (4096, 4096) and got.dtype == np.uint8
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (bad.size, [tuple(rgb.reshape(-1, 3)[i]) for i in bad[:4]])
    assert got[-1, -1] == 255 and got[0, 0] == 0  # white is exactly 255.0, black 0


def test_the_reference_tells_the_shortcuts_apart():
    """The integer form and the f32 form differ from the f64 expression on known numbers of triples: a comparison
    against gray_reference would catch either."""
    rgb = CC.all_triples()
    want = CC.all_triples_gray()
    d_int = np.flatnonzero(CC.gray_integer(rgb).ravel() != want.ravel())
    assert d_int.size == 1957
    assert tuple(int(v) for v in rgb.reshape(-1, 3)[d_int[0]]) == (0, 118, 66)
    n_f32 = 0
    for r in range(0, 4096, 512):
        n_f32 += int(np.count_nonzero(CC.gray_float32(rgb[r:r + 512]) != want[r:r + 512]))
    assert n_f32 == 2041


@pytest.mark.parametrize("width,rows,frames", [(1, 1, 1), (5, 3, 2), (64, 2, 3), (257, 3, 1)])
def test_host_strides_and_guards(width, rows, frames):
    """Padded row and frame strides (multiples of 4 and odd), both buffers at odd offsets: every byte of the destination
    outside the `width` bytes of each row keeps its guard value."""
    rng = np.random.default_rng(width * 7 + rows)
    for pad_row, pad_frame in ((0, 0), (4, 8), (3, 5)):
        srs, drs = 3 * width + pad_row, width + pad_row
        sfs, dfs = srs * rows + pad_frame, drs * rows + pad_frame
        src = rng.integers(0, 256, 3 + sfs * frames + 8, dtype=np.uint8)
        dst = np.full(5 + dfs * frames + 8, CC.GUARD, np.uint8)
        assert host(src, dst, width, rows, frames, (srs, sfs), (drs, dfs), 3, 5) == A.OK
        want = np.full_like(dst, CC.GUARD)
        for f in range(frames):
            for r in range(rows):
                px = src[3 + f * sfs + r * srs:][:3 * width].reshape(width, 3)
                want[5 + f * dfs + r * drs:][:width] = CC.gray_reference(px)
        assert np.array_equal(dst, want), (pad_row, pad_frame)
    # stride 0 means packed
    src = rng.integers(0, 256, (frames, rows, width, 3), dtype=np.uint8)
    dst = np.zeros((frames, rows, width), np.uint8)
    assert host(src, dst, width, rows, frames) == A.OK and np.array_equal(dst, CC.gray_reference(src))


def test_to_gray_host_takes_views():
    rng = np.random.default_rng(3)
    big = rng.integers(0, 256, (3, 6, 11, 3), dtype=np.uint8)
    view = big[:, 1:5, 2:9]
    assert np.array_equal(A.to_gray_host(view), CC.gray_reference(view))
    assert np.array_equal(A.to_gray_host(view[1]), CC.gray_reference(view[1]))
    assert np.array_equal(A.to_gray_host(big[:, :, ::-1]), CC.gray_reference(big[:, :, ::-1]))  # (copied first)
    with pytest.raises(ValueError):
        A.to_gray_host(big[..., :2])
    with pytest.raises(ValueError):
        A.to_gray_host(big.astype(np.uint16))


def test_host_refusals():
    src = np.zeros(3 * 8 * 4 * 2 + 64, np.uint8)
    dst = np.full(8 * 4 * 2 + 64, CC.GUARD, np.uint8)
    L = K.load()
    fn = L.adder_color_to_gray_host
    s, d = src.ctypes.data, dst.ctypes.data
    assert fn(None, 0, 0, d, 0, 0, 8, 4, 2) == A.E_BAD_PARAMS
    assert b"null" in L.adder_color_last_error()
    assert fn(s, 0, 0, None, 0, 0, 8, 4, 2) == A.E_BAD_PARAMS
    for w, r, f in ((0, 4, 2), (8, 0, 2), (8, 4, 0)):
        assert fn(s, 0, 0, d, 0, 0, w, r, f) == A.E_BAD_PARAMS
    assert b"zero extent" in L.adder_color_last_error()
    assert fn(s, 23, 0, d, 0, 0, 8, 4, 2) == A.E_BAD_PARAMS       # source row stride below 3 * width
    assert fn(s, 0, 0, d, 7, 0, 8, 4, 2) == A.E_BAD_PARAMS        # destination row stride below width
    assert fn(s, 0, 3 * 24 + 23, d, 0, 0, 8, 4, 2) == A.E_BAD_PARAMS  # source frame stride inside the frame before
    assert fn(s, 0, 0, d, 0, 31, 8, 4, 2) == A.E_BAD_PARAMS
    assert fn(s, 1 << 63, 0, d, 0, 0, 8, 4, 2) == A.E_BAD_PARAMS  # a range no address space holds
    # overlap: the destination inside the source's range, at its last byte, and the source inside the destination's
    buf = np.zeros(4 * 8 * 4 * 2 + 16, np.uint8)
    b = buf.ctypes.data
    n_src, n_dst = 3 * 8 * 4 * 2, 8 * 4 * 2
    assert fn(b, 0, 0, b + 5, 0, 0, 8, 4, 2) == A.E_BAD_PARAMS
    assert b"overlap" in L.adder_color_last_error()
    assert fn(b, 0, 0, b + n_src - 1, 0, 0, 8, 4, 2) == A.E_BAD_PARAMS
    assert fn(b + n_dst - 1, 0, 0, b, 0, 0, 8, 4, 2) == A.E_BAD_PARAMS
    assert (dst == CC.GUARD).all() and not buf.any()              # nothing was written by any refused call
    assert fn(b, 0, 0, b + n_src, 0, 0, 8, 4, 2) == A.OK          # back to back is fine
    assert fn(b + n_dst, 0, 0, b, 0, 0, 8, 4, 2) == A.OK


def test_binding_tables_match_the_headers():
    hdr = open(os.path.join(ROOT, "include", "adder_color.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(adder_color_\w+)\s*\(", hdr))
    assert names == set(K.SYMBOLS) and len(names) == 3
    L = A.load()
    for n in names:
        assert hasattr(L, n), n
    for n in ("adder_hip_integrate_rgb_device", "adder_hip_integrate_wire_rgb_device", "adder_hip_integrate_batch_rgb",
              "adder_hip_frame_submit_rgb"):
        assert n in A._native.SYMBOLS and hasattr(L, n), n
    host_lib = C.CDLL(os.path.join(ROOT, "adder-codec-rs_amd", "host", "libadder_host.so"))
    assert hasattr(host_lib, "adder_host_transcode_raw_ex")
