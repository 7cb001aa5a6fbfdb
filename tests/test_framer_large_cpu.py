"""The generator of the large-plane framer tests (tests/framer_large_stream.py) at a 64 x 33 twin shape, without a GPU:
the stream is what its description says, the holder of the minimum is unique and sits where asked, and the oracle fed
segment by segment answers as the oracle fed event by event."""
import numpy as np
import pytest

from oracle import oracle as O
import framer_large_stream as L
import kernel_constants

W, H = 64, 33
SPANS = (1024, 512, 2100)  # stand-ins for the grid caps inside the twin's 2112 units


@pytest.mark.parametrize("C,holder", [(1, W * H - 1), (1, 2100), (1, 0), (3, 3 * W * H - 1), (3, 2100)])
def test_stream_is_as_described_and_the_minimum_has_one_holder(C, holder):
    n = W * H * C
    ev, offs, lf, must = L.make_stream(W, H, C, holder, SPANS)
    assert {0, n - 1, 1023, 1024, 511, 512, 2099, 2100} <= set(must.tolist())
    unit = (ev["y"].astype(np.int64) * W + ev["x"]) * C + (0 if C == 1 else ev["c"])
    seg = [unit[int(offs[k]):int(offs[k + 1])] for k in range(3)]
    assert np.array_equal(seg[0], np.arange(n))                       # every unit once
    assert all((np.diff(s) > 0).all() for s in seg)                   # raster order, a unit at most once a segment
    assert 0.27 < len(seg[1]) / n < 0.33 and 0.03 < len(seg[2]) / n < 0.08
    assert np.isin(must, seg[2]).all() and holder not in seg[1]
    assert set(np.unique(ev["t"]).tolist()) <= {0, 255, 510, 765} and ev["d"].max() == 8 and ev["d"].min() == 0
    zero_t = np.flatnonzero(ev["t"] == 0)
    assert len(zero_t) == (1 if holder in must else 0) and (unit[zero_t] == holder).all()
    assert set(np.unique(lf[0]).tolist()) == {0, 1, 2} and lf[2].max() <= 8 and lf[2].max() >= 6
    # one holder of the minimum, where asked; everything else is at least a frame ahead
    assert lf[2][holder] == 0 and np.count_nonzero(lf[2] == 0) == 1 and np.count_nonzero(lf[0] == 0) > 1
    # a unit's last_filled as the oracle counts it: 1 complete frame after segment 0, and still 1 at the end
    fr = L.new_oracle(W, H, C)
    L.oracle_ingest(fr, ev, offs, 0)
    assert fr.is_frame_filled(0) and not fr.is_frame_filled(1)
    L.oracle_ingest(fr, ev, offs, 1)
    L.oracle_ingest(fr, ev, offs, 2)
    assert fr.is_frame_filled(0) and not fr.is_frame_filled(1)
    ready = fr.write_multi_frame_bytes(max_frames=L.RING_FRAMES)
    assert len(ready) == n and fr.frames_written == 1
    # the masked hand-out: exactly the units that reached frame 1 have a value there
    nxt = np.frombuffer(fr.write_frame_bytes(), np.uint8)
    assert not nxt[lf[2] < 1].any() and np.count_nonzero(nxt) > n // 2


@pytest.mark.parametrize("value_type", [0, 1, 2])
def test_segment_feed_equals_the_event_by_event_oracle(value_type):
    C, holder = 1, 2100
    ev, offs, steps = L.case(W, H, C, holder, value_type, SPANS)
    fr = L.new_oracle(W, H, C, value_type)
    ready = fr.ingest_events(ev)  # pops complete frames where the reference's read loop does
    assert len(ready) == (W * H * C) << value_type
    rest = L.hand_out(fr, lambda f: b"")[1:]
    assert steps[0] == ("ready frames", ready, 1) and steps[1:] == rest
    assert [s[2] for s in steps] == [1, 2, 3, 3, 4, 5] and steps[3][1] is True
    assert all(len(s[1]) == len(ready) for s in steps if s[0] != "flush_frame_buffer")


def test_large_planes_sit_past_the_grid_caps():
    import test_gpu_framer_large as T
    pop, wide, mm = L.grid_spans(kernel_constants.framer())
    (w1, h1, c1), (w2, h2, c2), (w3, h3, c3) = T.U8_PLANES
    assert pop < w1 * h1 * c1 <= pop + w1 and (w1 * h1 * c1) % 4 == 0      # a second pass of the 4-byte path
    assert pop < w2 * h2 * c2 and (w2 * h2 * c2) % 4 != 0                 # ... and of the byte path
    assert mm < w3 * h3 * c3 <= mm + w3 * c3 and c3 == 3                  # past the min / max cap
    ww, wh, wc = T.WIDE_PLANE
    assert wide < ww * wh * wc <= wide + ww
    if (pop, wide, mm) == (2097152, 524288, 4194304):
        assert T.U8_PLANES == ((2048, 1025, 1), (2049, 1025, 1), (2048, 683, 3)) and T.WIDE_PLANE == (1024, 513, 1)
