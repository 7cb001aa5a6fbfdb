"""The framer's hand-out kernels (csrc/adder_framer_kernels.hip) on planes past their grid caps: the u8 pop's
grid-stride pass on its 4-byte and its byte path, the u16 / u32 pop past its cap's first pass, a min / max that has to
see units past its cap for frames_ready to be right -- at the size of the 1080p RGB streams the transcoder produces.
The planes follow the constants of csrc/adder_framer_kernels.h; the stream and the oracle's answers come from
tests/framer_large_stream.py (checked on the CPU in tests/test_framer_large_cpu.py).  Everything is compared with
oracle.Framer byte for byte."""
import numpy as np
import pytest

import framer_large_stream as L

pytestmark = pytest.mark.gpu

POP_SPAN, WIDE_SPAN, MINMAX_SPAN = L.grid_spans()
# just past a pass of the u8 pop at its cap (a multiple of 4 units, then an odd count), and of the min / max (RGB)
U8_PLANES = ((2048, POP_SPAN // 2048 + 1, 1), (2049, POP_SPAN // 2048 + 1, 1), (2048, MINMAX_SPAN // (2048 * 3) + 1, 3))
WIDE_PLANE = (1024, WIDE_SPAN // 1024 + 1, 1)
LAST = -1  # the holder of the minimum at the plane's last unit


def _hip():
    import adder_amd
    return adder_amd


def _ingest(fr, path, d_ev, offs, st):
    import torch
    if path == "segments":   # one launch per segment
        fr.ingest_device(d_ev, offs, stream=st)
    elif path == "tiles":    # the tile kernel (u16 / u32: the library sends it through the segment kernel)
        fr.ingest_frames_device(d_ev, offs, stream=st)
    else:                    # the tile kernel with the offsets on the device
        d_off = torch.from_numpy(offs.astype(np.int64)).cuda()
        fr.ingest_frames_device_offsets(d_ev, d_off, len(offs) - 1, stream=st)


def _run(W, H, C, holder, path, value_type=0):
    import torch
    A = _hip()
    ev, offs, want = L.case(W, H, C, holder, value_type)
    n_units = W * H * C
    fb = n_units << value_type
    n_ready = len(want[0][1]) // fb
    assert n_ready == 1 and len(want[0][1]) == fb
    st = torch.cuda.current_stream().cuda_stream
    d_ev = torch.from_numpy(ev.view(np.uint8).reshape(-1, 12)).cuda()
    kw = dict(time_mode=A.TIME_DELTA_T, source_camera=A.FRAMED_U8, ring_frames=L.RING_FRAMES, value_type=value_type,
              **L.FRAMER_KW)

    fr = A.HipFramer(W, H, C, **kw)
    assert fr.tpf == L.TPF and fr.frame_bytes == fb
    _ingest(fr, path, d_ev, offs, st)
    assert fr.frames_ready() == n_ready  # (more: the min / max missed the one unit that holds the minimum)
    got = L.hand_out(fr, lambda f: f.pop(max_frames=f.frames_ready()))
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[2] == w[2], (g[0], g[2], w[2])
        if g[1] != w[1]:
            a, b = np.frombuffer(g[1], np.uint8), np.frombuffer(w[1], np.uint8)
            bad = np.flatnonzero(a != b) if len(a) == len(b) else None
            raise AssertionError((g[0], len(a), len(b), None if bad is None else (len(bad), bad[:8], bad[-8:])))
    fr.close()

    # a second context: the complete frames handed out on the device
    fr2 = A.HipFramer(W, H, C, **kw)
    _ingest(fr2, path, d_ev, offs, st)
    d_out = torch.full((2 * fb,), 0xA5, dtype=torch.uint8, device="cuda")
    assert fr2.pop_device(d_out, 2, stream=st) == n_ready and fr2.frames_written == n_ready
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert out[:fb].tobytes() == want[0][1] and (out[fb:] == 0xA5).all()
    assert fr2.frames_ready() == 0
    fr2.close()


@pytest.mark.parametrize("plane,holder,path", [
    (0, LAST, "segments"), (0, LAST, "tiles"), (1, LAST, "segments"), (1, LAST, "tiles"),
    (2, LAST, "segments"), (2, LAST, "tiles"),
    (2, MINMAX_SPAN, "segments"), (2, MINMAX_SPAN, "tiles"), (2, MINMAX_SPAN, "device offsets")])
def test_u8_planes_past_the_pop_and_minmax_caps(plane, holder, path):
    _run(*U8_PLANES[plane], holder, path)


@pytest.mark.parametrize("path", ["segments", "tiles"])
@pytest.mark.parametrize("value_type", [1, 2])
def test_u16_u32_plane_past_the_pop_cap(value_type, path):
    _run(*WIDE_PLANE, LAST, path, value_type)
