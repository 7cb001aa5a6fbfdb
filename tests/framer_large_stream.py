"""The event stream of the large-plane framer tests (tests/test_gpu_framer_large.py) and the framer oracle's answers
to it; vectorised numpy, checked on the CPU at a small twin shape (tests/test_framer_large_cpu.py).

Three raster-ordered DeltaT segments, 255 ticks per output frame (tps 7650, ref_interval 255, 30 fps):
  0: every unit one event, d in 0 .. 8, t in {255, 510, 765}: last_filled becomes 0, 1 or 2;
  1: a random 30 % of the units one more event;
  2: about 5 % one more: unit 0, the last unit, the units on both sides of every grid-cap boundary (`spans`), every
     unit still at frame 0, and random ones.
One unit, the holder, is the only one left at frame 0, so exactly one frame is complete: a min / max that misses the
holder reports more.  Where segment 2 has to include the holder, its event there carries t = 0, which moves nothing.
No unit gets past frame 8, so a ring of 16 frames holds everything."""
import functools

import numpy as np

from oracle import oracle as O
import kernel_constants

FRAMER_KW = dict(tps=7650, ref_interval=255, delta_t_max=7650, output_fps=30.0, codec_version=3)
TPF = 255
RING_FRAMES = 16
CHUNK_ROWS = 64


def grid_spans(k=None):
    """Units one pass of each hand-out kernel covers at its grid cap: (u8 pop, u16 / u32 pop, min / max)."""
    k = k or kernel_constants.framer()
    return (k["kFramerPopMaxBlocks"] * k["kFramerPopUnitsPerBlock"],
            k["kFramerPopMaxBlocks"] * k["kFramerPopWideUnitsPerBlock"],
            k["kFramerMinmaxMaxBlocks"] * k["kFramerMinmaxUnitsPerBlock"])


def _events(units, d, t, W, C):
    ev = np.zeros(len(units), O.EVENT_DTYPE)
    ev["c"] = 0xFF if C == 1 else units % C
    ev["x"] = (units // C) % W
    ev["y"] = units // (C * W)
    ev["d"] = d
    ev["t"] = t
    return ev


def make_stream(W, H, C, holder, spans, seed=1):
    """-> (events, offsets [4], last_filled [n_units] after each segment [3][n_units], must: the units segment 2 has to
    include).  holder: the unit that alone stays at frame 0."""
    n = W * H * C
    rng = np.random.default_rng(seed)
    ticks = np.array([255, 510, 765])
    must = np.unique(np.array([0, n - 1] + [u for s in spans if s < n for u in (s - 1, s)], np.int64))

    t0 = rng.choice(ticks, n, p=[0.02, 0.49, 0.49])
    t0[holder] = 255
    ts = t0.astype(np.int64)
    segs = [_events(np.arange(n), rng.integers(0, 9, n), t0, W, C)]
    lf = [(ts - 1) // TPF]

    pick = rng.random(n) < 0.30
    pick[holder] = False
    u1 = np.flatnonzero(pick)
    t1 = rng.choice(ticks, len(u1))
    ts[u1] += t1
    segs.append(_events(u1, rng.integers(0, 9, len(u1)), t1, W, C))
    lf.append((ts - 1) // TPF)

    pick = (rng.random(n) < 0.036) | (lf[1] == 0)
    pick[must] = True
    pick[holder] = bool((must == holder).any())
    u2 = np.flatnonzero(pick)
    t2 = rng.choice(ticks, len(u2))
    t2[u2 == holder] = 0
    ts[u2] += t2
    segs.append(_events(u2, rng.integers(0, 9, len(u2)), t2, W, C))
    lf.append((ts - 1) // TPF)

    offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
    return np.concatenate(segs), offs, np.stack(lf), must


def new_oracle(W, H, C, value_type=0):
    fr = O.Framer(W, H, C, chunk_rows=CHUNK_ROWS, time_mode=O.DELTA_T, source_camera=O.FRAMED_U8, **FRAMER_KW)
    if value_type:
        fr.set_value_type(value_type)
    return fr


def oracle_ingest(fr, ev, offs, seg):
    """One raster-ordered segment into the oracle through ingest_events_events: its rows are already grouped by chunk."""
    e = ev[int(offs[seg]):int(offs[seg + 1])]
    bounds = np.arange(fr.num_chunks + 1, dtype=np.int64) * fr.chunk_rows
    fr.ingest_events_events(e, np.searchsorted(e["y"], bounds, side="left").astype(np.uint64))


def hand_out(fr, pop_ready):
    """The hand-out sequence of the tests on the oracle or on a HipFramer (same method names but for the pop of the
    complete frames, `pop_ready`): -> [(step, value, frames_written)]."""
    steps = [("ready frames", pop_ready(fr), fr.frames_written)]
    for k in (0, 1):  # incomplete frames: units without a value read 0
        steps.append((f"write_frame_bytes {k}", fr.write_frame_bytes(), fr.frames_written))
    steps.append(("flush_frame_buffer", fr.flush_frame_buffer(), fr.frames_written))
    for k in (2, 3):  # the flushed frame, whole; then an incomplete one again
        steps.append((f"write_frame_bytes {k}", fr.write_frame_bytes(), fr.frames_written))
    return steps


@functools.lru_cache(maxsize=2)
def case(W, H, C, holder, value_type=0, spans=None):
    """-> (events, offsets, the oracle's hand_out steps) of a plane; holder < 0 counts from the plane's end."""
    n = W * H * C
    ev, offs, _, _ = make_stream(W, H, C, holder % n, spans or grid_spans())
    fr = new_oracle(W, H, C, value_type)
    for seg in range(3):
        oracle_ingest(fr, ev, offs, seg)
    return ev, offs, hand_out(fr, lambda f: f.write_multi_frame_bytes(max_frames=RING_FRAMES))
