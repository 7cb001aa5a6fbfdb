"""The colour-to-gray kernel (include/adder_color.h) and the *_rgb entry points of include/adder_hip.h on the device:
all 2^24 triples, the dword / byte paths at their edges with guard bytes around every row, the grid clamp, the refusals,
and colour frames through a one-channel context against the gray twin and the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import adder_amd as A
from adder_amd import color as K
from oracle import oracle as O

import color_cases as CC

DEV = "cuda:0"
T = 20
CRFS = (0, 3)  # crf 0 and the default quality (Crf::new(None): quality 3)


def torch_():
    import torch
    return torch


# ---------------------------------------------------------------- the kernel

def test_device_equals_the_reference_on_every_triple():
    torch = torch_()
    i = torch.arange(1 << 24, dtype=torch.int32, device=DEV)
    rgb = torch.stack((i >> 16, (i >> 8) & 255, i & 255), dim=1).to(torch.uint8).reshape(4096, 4096, 3)
    got = A.to_gray_device(rgb)
    want = torch.from_numpy(np.array(CC.all_triples_gray())).to(DEV)
    bad = torch.nonzero(got.reshape(-1) != want.reshape(-1)).reshape(-1)
    assert bad.numel() == 0, (int(bad.numel()), [tuple(rgb.reshape(-1, 3)[int(k)].tolist()) for k in bad[:4]])
    assert int(got[-1, -1]) == 255 and int(got[0, 0]) == 0


def _strides(width, rows, kind):
    """(src row, src frame, dst row, dst frame) in bytes: packed, padded to multiples of 4, padded and odd."""
    if kind == "packed":
        srs, drs = 3 * width, width
        return srs, srs * rows, drs, drs * rows
    if kind == "pad4":
        srs, drs = (3 * width + 3) // 4 * 4 + 4, (width + 3) // 4 * 4 + 8
        return srs, srs * rows + 12, drs, drs * rows + 4
    srs, drs = (3 * width + 6) | 1, (width + 2) | 1
    return srs, (srs * rows + 8) | 1, drs, (drs * rows + 4) | 1


@pytest.mark.parametrize("width", CC.EDGE_WIDTHS)
def test_edges_strides_phases_and_guards(width):
    """Rows of 1 .. 1021 pixels, 1 to 3 rows and frames, three stride arrangements, source and destination at every byte
    phase: the gray bytes are the reference's and every other byte of the destination buffer keeps its guard value."""
    torch = torch_()
    rng = np.random.default_rng(width)
    lead = 8  # guard bytes in front of the first row (a multiple of 4: the phase stays the phase)
    for rows in (1, 2, 3):
        for frames in (1, 2, 3):
            rgb = rng.integers(0, 256, (frames, rows, width, 3), dtype=np.uint8)
            d_rgb = torch.from_numpy(rgb).to(DEV)
            d_want_gray = torch.from_numpy(CC.gray_reference(rgb)).to(DEV)
            for kind in ("packed", "pad4", "odd"):
                srs, sfs, drs, dfs = _strides(width, rows, kind)
                src_buf = torch.randint(0, 256, (lead + 4 + sfs * frames + 16,), dtype=torch.uint8, device=DEV)
                dst_buf = torch.empty(lead + 4 + dfs * frames + 16, dtype=torch.uint8, device=DEV)
                want_buf = torch.empty_like(dst_buf)
                assert src_buf.data_ptr() % 4 == 0 and dst_buf.data_ptr() % 4 == 0
                for sp in range(4):
                    src = torch.as_strided(src_buf, (frames, rows, width, 3), (sfs, srs, 3, 1), lead + sp)
                    src.copy_(d_rgb)
                    for dp in range(4):
                        dst_buf.fill_(CC.GUARD)
                        want_buf.fill_(CC.GUARD)
                        dst = torch.as_strided(dst_buf, (frames, rows, width), (dfs, drs, 1), lead + dp)
                        torch.as_strided(want_buf, (frames, rows, width), (dfs, drs, 1), lead + dp).copy_(d_want_gray)
                        assert dst.data_ptr() % 4 == dp and src.data_ptr() % 4 == sp
                        A.to_gray_device(src, dst)
                        assert torch.equal(dst_buf, want_buf), (rows, frames, kind, sp, dp)


@pytest.mark.parametrize("width,rows,frames", [(4 * 64 * 64 + 261, 3, 2), (5, 1027, 70)])
def test_past_the_grid_clamp(width, rows, frames):
    """More lanes' worth of a row than the clamped grid is wide (64 blocks of 64 lanes of 4 pixels); more rows than its
    256 blocks of 4 rows and more frames than the blocks the plane leaves (16384 / 256 = 64): the strided loops."""
    torch = torch_()
    rng = np.random.default_rng(rows)
    rgb = rng.integers(0, 256, (frames, rows, width, 3), dtype=np.uint8)
    d_gray = torch.full((frames, rows, width + 3), CC.GUARD, dtype=torch.uint8, device=DEV)
    A.to_gray_device(torch.from_numpy(rgb).to(DEV), d_gray[:, :, :width])
    got = d_gray.cpu().numpy()
    assert np.array_equal(got[:, :, :width], CC.gray_reference(rgb)) and (got[:, :, width:] == CC.GUARD).all()


def test_device_refusals():
    torch = torch_()
    L = K.load()
    fn = L.adder_color_to_gray_device
    src = torch.zeros(3 * 8 * 4 * 2 + 64, dtype=torch.uint8, device=DEV)
    dst = torch.full((8 * 4 * 2 + 64,), CC.GUARD, dtype=torch.uint8, device=DEV)
    s, d = src.data_ptr(), dst.data_ptr()
    bad = A.E_BAD_PARAMS
    assert fn(None, 0, 0, d, 0, 0, 8, 4, 2, None) == bad and fn(s, 0, 0, None, 0, 0, 8, 4, 2, None) == bad
    assert b"null" in L.adder_color_last_error()
    for w, r, f in ((0, 4, 2), (8, 0, 2), (8, 4, 0)):
        assert fn(s, 0, 0, d, 0, 0, w, r, f, None) == bad
    assert fn(s, 23, 0, d, 0, 0, 8, 4, 2, None) == bad        # row strides below a row
    assert fn(s, 0, 0, d, 7, 0, 8, 4, 2, None) == bad
    assert fn(s, 0, 95, d, 0, 0, 8, 4, 2, None) == bad        # frame strides inside the frame before
    assert fn(s, 0, 0, d, 0, 31, 8, 4, 2, None) == bad
    n_src, n_dst = 3 * 8 * 4 * 2, 8 * 4 * 2
    buf = torch.zeros(n_src + n_dst + 16, dtype=torch.uint8, device=DEV)
    b = buf.data_ptr()
    assert fn(b, 0, 0, b + 5, 0, 0, 8, 4, 2, None) == bad     # overlap
    assert b"overlap" in L.adder_color_last_error()
    assert fn(b, 0, 0, b + n_src - 1, 0, 0, 8, 4, 2, None) == bad
    assert fn(b + n_dst - 1, 0, 0, b, 0, 0, 8, 4, 2, None) == bad
    torch.cuda.synchronize()
    assert bool((dst == CC.GUARD).all()) and not bool(buf.any())  # nothing was queued by a refused call
    assert fn(b, 0, 0, b + n_src, 0, 0, 8, 4, 2, None) == A.OK   # back to back is fine
    torch.cuda.synchronize()


# ---------------------------------------------------------------- colour frames through a one-channel context

def _clip(width, height, seed):
    return np.random.default_rng(seed).integers(0, 256, (T, height, width, 3), dtype=np.uint8)


def _video(width, height, crf, band=None, **kw):
    """-> (a HipVideo of one channel, the oracle's Video over the same rows), both at quality `crf`."""
    y0, y1 = band or (0, height)
    base, cmax, vel = A.CRF[crf]
    hv = A.HipVideo(width, height, 1, row_begin=y0, row_end=y1, **kw)
    hv.set_crf_parameters(cmax, vel)
    hv.reset_c_thresh(base)
    ov = O.Video(width, y1 - y0, 1, row_begin=y0)
    ov.set_crf_parameters(cmax, vel)
    ov.reset_c_thresh(base)
    ov.ensure_capacity(18)
    return hv, ov


def _oracle(ov, gray):
    """-> (events of all frames, frame offsets)."""
    per = [ov.integrate_matrix(g) for g in gray]
    return np.concatenate(per), np.cumsum([0] + [len(p) for p in per]).astype(np.uint64)


def _device_batch(hv, d_frames, rgb, wire=False, cap=None, stream=True):
    """One device batch (colour or gray frames) -> (events or wire bytes, offsets)."""
    torch = torch_()
    n_frames = d_frames.shape[0]
    cap = hv.max_events_per_frame * n_frames if cap is None else cap
    rec = 9 if wire else 12
    d_out = torch.empty(max(cap * rec, 16), dtype=torch.uint8, device=DEV)
    d_offs = torch.zeros(n_frames + 1, dtype=torch.int64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream if stream else None
    fn = {(False, False): hv.integrate_device, (False, True): hv.integrate_wire_device,
          (True, False): hv.integrate_rgb_device, (True, True): hv.integrate_wire_rgb_device}[(rgb, wire)]
    fn(d_frames, d_out, d_offs, stream=s)
    n = hv.finish()
    out = d_out[: n * rec].cpu().numpy()
    return (out.tobytes() if wire else np.frombuffer(out.tobytes(), dtype=A.EVENT_DTYPE)), d_offs.cpu().numpy().astype(np.uint64)


PLANES = [(14, 9), (70, 33)]


@pytest.mark.parametrize("crf", CRFS)
@pytest.mark.parametrize("width,height", PLANES)
def test_integrate_rgb_device(width, height, crf):
    torch = torch_()
    rgb = _clip(width, height, 1)
    gray = A.to_gray_host(rgb)
    hv, ov = _video(width, height, crf)
    hv2, _ = _video(width, height, crf)
    want, want_offs = _oracle(ov, gray)
    got, offs = _device_batch(hv, torch.from_numpy(rgb).to(DEV), True)
    twin, twin_offs = _device_batch(hv2, torch.from_numpy(gray.reshape(T, -1)).to(DEV), False)
    assert len(want) > 0 and np.array_equal(got, twin) and np.array_equal(offs, twin_offs)
    assert np.array_equal(got, want) and np.array_equal(offs, want_offs)


@pytest.mark.parametrize("crf", CRFS)
@pytest.mark.parametrize("width,height", PLANES)
def test_integrate_wire_rgb_device(width, height, crf):
    torch = torch_()
    rgb = _clip(width, height, 2)
    gray = A.to_gray_host(rgb)
    hv, ov = _video(width, height, crf)
    hv2, _ = _video(width, height, crf)
    want, want_offs = _oracle(ov, gray)
    got, offs = _device_batch(hv, torch.from_numpy(rgb).to(DEV), True, wire=True)
    twin, twin_offs = _device_batch(hv2, torch.from_numpy(gray.reshape(T, -1)).to(DEV), False, wire=True)
    assert got == twin and np.array_equal(offs, twin_offs)
    assert got == A.raw_events(want, 1) and np.array_equal(offs, want_offs)


@pytest.mark.parametrize("crf", CRFS)
@pytest.mark.parametrize("width,height", PLANES)
def test_integrate_batch_rgb(width, height, crf):
    rgb = _clip(width, height, 3)
    gray = A.to_gray_host(rgb)
    hv, ov = _video(width, height, crf)
    hv2, _ = _video(width, height, crf)
    want, want_offs = _oracle(ov, gray)
    got, offs = hv.integrate_batch_rgb(rgb)
    twin, twin_offs = hv2.integrate_batch(gray)
    assert np.array_equal(got, twin) and np.array_equal(offs, twin_offs)
    assert np.array_equal(got, want) and np.array_equal(offs, want_offs)
    # the same frames as a view with padded rows and frames: passed with its strides
    hv3, _ = _video(width, height, crf)
    big = np.zeros((T, height + 1, width + 3, 3), np.uint8)
    big[:, :height, :width] = rgb
    got3, offs3 = hv3.integrate_batch_rgb(big[:, :height, :width])
    assert np.array_equal(got3, want) and np.array_equal(offs3, want_offs)


@pytest.mark.parametrize("crf", CRFS)
@pytest.mark.parametrize("width,height", PLANES)
def test_frame_submit_rgb(width, height, crf):
    rgb = _clip(width, height, 4)
    gray = A.to_gray_host(rgb)
    hv, ov = _video(width, height, crf)
    hv2, _ = _video(width, height, crf)
    for k in range(T):
        want, want_chunks = ov.integrate_matrix(gray[k], want_chunks=True)
        hv.frame_submit_rgb(rgb[k])
        got, chunks = hv.frame_collect(want_chunks=True)
        hv2.frame_submit(gray[k])
        twin, twin_chunks = hv2.frame_collect(want_chunks=True)
        assert np.array_equal(got, twin) and np.array_equal(chunks, twin_chunks), k
        assert np.array_equal(got, want) and np.array_equal(chunks, want_chunks), k


def test_row_band_context():
    """A context that owns rows 3..7 of 9 takes its own rows of the colour frames, through all four entry points."""
    torch = torch_()
    width, height, band = 14, 9, (3, 7)
    rgb = _clip(width, height, 5)[:, band[0]:band[1]]
    gray = A.to_gray_host(rgb)
    _, ov = _video(width, height, 0, band)
    want, want_offs = _oracle(ov, gray)
    hv, _ = _video(width, height, 0, band)
    got, offs = _device_batch(hv, torch.from_numpy(np.ascontiguousarray(rgb)).to(DEV), True)
    assert np.array_equal(got, want) and np.array_equal(offs, want_offs) and want["y"].min() >= 3 and want["y"].max() < 7
    hv, _ = _video(width, height, 0, band)
    got, offs = _device_batch(hv, torch.from_numpy(np.ascontiguousarray(rgb)).to(DEV), True, wire=True)
    assert got == A.raw_events(want, 1) and np.array_equal(offs, want_offs)
    hv, _ = _video(width, height, 0, band)
    got, offs = hv.integrate_batch_rgb(rgb)  # (a view of the full frames: rows 3..7, passed with its frame stride)
    assert np.array_equal(got, want) and np.array_equal(offs, want_offs)
    hv, _ = _video(width, height, 0, band)
    per = []
    for k in range(T):
        hv.frame_submit_rgb(rgb[k])
        per.append(hv.frame_collect())
    assert np.array_equal(np.concatenate(per), want)


def test_out_cap_too_small_rolls_back_and_the_retry_succeeds():
    torch = torch_()
    width, height = 70, 33
    rgb = _clip(width, height, 6)
    gray = A.to_gray_host(rgb)
    _, ov = _video(width, height, 3)
    want, want_offs = _oracle(ov, gray)
    d_rgb = torch.from_numpy(rgb).to(DEV)
    hv, _ = _video(width, height, 3)
    with pytest.raises(A.AdderHipError) as ei:
        _device_batch(hv, d_rgb, True, cap=len(want) // 2)
    assert ei.value.code == A.E_OUT_CAPACITY and hv.last_required == len(want)
    got, offs = _device_batch(hv, d_rgb, True, cap=hv.last_required)
    assert np.array_equal(got, want) and np.array_equal(offs, want_offs)
    hv, _ = _video(width, height, 3)
    with pytest.raises(A.AdderHipError) as ei:
        hv.integrate_batch_rgb(rgb, out_cap=len(want) // 2)
    assert ei.value.code == A.E_OUT_CAPACITY and hv.last_required == len(want)
    got, offs = hv.integrate_batch_rgb(rgb, out_cap=hv.last_required)
    assert np.array_equal(got, want) and np.array_equal(offs, want_offs)


def test_ring_three_frames_in_flight_with_padded_rows():
    width, height = 70, 33
    rgb = _clip(width, height, 7)
    gray = A.to_gray_host(rgb)
    hv, ov = _video(width, height, 3)
    want = [ov.integrate_matrix(g) for g in gray]
    padded = np.full((T, height, width * 3 + 5), 0x5A, np.uint8)  # rows of 3 * width + 5 bytes
    frames = padded[:, :, : width * 3].reshape(T, height, width, 3)
    frames[...] = rgb
    assert frames.strides[1] == width * 3 + 5 and np.shares_memory(frames, padded)
    hv.frames_configure(3)
    got = []
    for k in range(3):
        hv.frame_submit_rgb(frames[k])
    assert hv.frames_in_flight() == 3
    with pytest.raises(A.AdderHipError):  # the ring is full, as for the gray twin
        hv.frame_submit_rgb(frames[3])
    for k in range(3, T):
        got.append(hv.frame_collect())
        hv.frame_submit_rgb(frames[k])
        assert hv.frames_in_flight() == 3
    while hv.frames_in_flight():
        got.append(hv.frame_collect())
    assert len(got) == T
    for k in range(T):
        assert np.array_equal(got[k], want[k]), k


def test_two_batches_back_to_back_on_the_null_stream():
    """stream == NULL: what the caller queued on the default stream just before the call -- here the batch's colour
    frames and the zeroed offsets -- is seen by the conversion and by the batch behind it."""
    torch = torch_()
    width, height = 70, 33
    a, b = _clip(width, height, 8), _clip(width, height, 9)
    hv, ov = _video(width, height, 0)
    want_a, offs_a = _oracle(ov, A.to_gray_host(a))
    want_b, offs_b = _oracle(ov, A.to_gray_host(b))
    d_a, d_b = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    cap = hv.max_events_per_frame * T
    d_in = torch.empty_like(d_a)
    d_out = torch.empty(cap * 12, dtype=torch.uint8, device=DEV)
    d_offs = torch.empty(T + 1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    for d_src, want, want_offs in ((d_a, want_a, offs_a), (d_b, want_b, offs_b)):
        d_offs.fill_(-1)
        d_in.copy_(d_src)  # on the default stream, not waited for
        hv.integrate_rgb_device(d_in, d_out, d_offs, stream=None)
        n = hv.finish()
        got = np.frombuffer(d_out[: n * 12].cpu().numpy().tobytes(), dtype=A.EVENT_DTYPE)
        assert np.array_equal(got, want) and np.array_equal(d_offs.cpu().numpy().astype(np.uint64), want_offs)


def test_three_channel_context_refuses_every_rgb_entry_point():
    torch = torch_()
    width, height = 14, 9
    rgb = _clip(width, height, 10)
    hv = A.HipVideo(width, height, 3)
    hv.set_crf_parameters(0, 10)
    hv.reset_c_thresh(0)
    d_rgb = torch.from_numpy(rgb.reshape(T, -1)).to(DEV)
    d_out = torch.empty(hv.max_events_per_frame * T * 12, dtype=torch.uint8, device=DEV)
    d_offs = torch.zeros(T + 1, dtype=torch.int64, device=DEV)
    L, h = hv.L, hv.h
    n = C.c_size_t(0)
    offs = np.zeros(T + 1, np.uint64)
    out = np.zeros(16, A.EVENT_DTYPE)
    assert L.adder_hip_integrate_rgb_device(h, d_rgb.data_ptr(), T, 255.0, d_out.data_ptr(), 16, d_offs.data_ptr(), None) == A.E_BAD_PARAMS
    assert b"channels == 1" in L.adder_hip_last_error(h)
    assert L.adder_hip_integrate_wire_rgb_device(h, d_rgb.data_ptr(), T, 255.0, d_out.data_ptr(), 160, d_offs.data_ptr(), None) == A.E_BAD_PARAMS
    assert L.adder_hip_integrate_batch_rgb(h, rgb.ctypes.data, T, 0, 0, 255.0, out.ctypes.data, 16, C.byref(n), offs.ctypes.data) == A.E_BAD_PARAMS
    assert L.adder_hip_frame_submit_rgb(h, rgb.ctypes.data, 0, 255.0) == A.E_BAD_PARAMS
    assert hv.frames_in_flight() == 0
    with pytest.raises(A.AdderHipError):  # nothing is pending
        hv.finish()
    # the context is as it was: its own colour batch equals the oracle's
    ov = O.Video(width, height, 3)
    ov.set_crf_parameters(0, 10)
    ov.reset_c_thresh(0)
    ov.ensure_capacity(18)
    want, want_offs = _oracle(ov, rgb)
    hv.integrate_device(d_rgb, d_out, d_offs, stream=torch.cuda.current_stream().cuda_stream)
    n_ev = hv.finish()
    got = np.frombuffer(d_out[: n_ev * 12].cpu().numpy().tobytes(), dtype=A.EVENT_DTYPE)
    assert np.array_equal(got, want) and np.array_equal(d_offs.cpu().numpy().astype(np.uint64), want_offs)


# ---------------------------------------------------------------- the C++ mirror

def _transcode_ex(frames, out_path, convert_on_device, crf):
    import host_py as Hst
    L = Hst.lib()
    fn = L.adder_host_transcode_raw_ex
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_int, C.c_uint32,
                   C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_char_p, C.POINTER(C.c_uint32), C.c_int, C.c_void_p,
                   C.POINTER(C.c_double)]
    frames = np.ascontiguousarray(frames, np.uint8)
    n_frames, height, width, cin = frames.shape
    last = np.zeros((height, width), np.uint8)
    chunks, secs = C.c_uint32(0), C.c_double(0.0)
    n = fn(frames.ctypes.data, n_frames, width, height, cin, 0, 30.0, crf, 255, 510, 1, 1, 1, -1, out_path.encode(),
           C.byref(chunks), int(convert_on_device), last.ctypes.data, C.byref(secs))
    assert n >= 0, Hst.err()
    return n, last, open(out_path, "rb").read()


@pytest.mark.parametrize("crf", [0, -1])
def test_mirror_convert_on_device(tmp_path, crf):
    import host_py as Hst
    rgb = np.random.default_rng(0).integers(0, 256, (T, 9, 14, 3), dtype=np.uint8)
    n_off, in_off, bytes_off = _transcode_ex(rgb, str(tmp_path / "off.adder"), False, crf)
    n_on, in_on, bytes_on = _transcode_ex(rgb, str(tmp_path / "on.adder"), True, crf)
    assert n_on == n_off > 0 and bytes_on == bytes_off
    gray_last = CC.gray_reference(rgb[-1])
    assert np.array_equal(in_off, gray_last) and np.array_equal(in_on, gray_last)
    n_old, _ = Hst.transcode_raw(rgb, color_input=False, crf=crf, ref_time=255, delta_t_max=510, time_mode=1, multi_mode=1,
                                 out_path=str(tmp_path / "old.adder"))
    assert n_old == n_on and open(str(tmp_path / "old.adder"), "rb").read() == bytes_on
