"""The HIP framer with frame rings that wrap (slot = frame % ring_frames), above all the tile kernel behind
ingest_frames_device: its ring_slot (a fast_div by the ring size), its K-row LDS window at F & (K - 1), the row_ok
guard and the single-byte stores of stragglers.  K is the window depth adder_framer_create chooses: 16 rows, or 32 when
delta_t_max / tpf + 4 (AbsoluteT) or + 24 (DeltaT) passes 16 -- with delta_t_max = 255 and 255 ticks per frame that is
16 for AbsoluteT and 32 for DeltaT streams.  Rings: 5 (below K), K itself, and K + 5 (above K, no multiple of it, no
power of two: 21 and 37).

The loop is that of test_gpu_framer_fuzz.py (O.Video events per source frame, O.Framer.ingest_events as the reference,
pop after every ingest, the flush / write_frame_bytes epilogue) on a fixed set of cases.  Which source frames make a
batch is decided by arithmetic on the events alone (the per-unit clock of ingest_event_for_chunk, unit_chain): a batch
is extended while its fills stay below frames_written + ring, and is capped by a fixed pattern (the whole ring, then a
few frames) so that batches start at every slot and straddle the end of the ring.  Every case passes the ring at least
three times; a ring-overflow error from a planned batch is a failure.  u16 / u32 frames and detect_features go through
the per-event kernels (adder_framer_segment_kernel, adder_framer_features.hip), which fill the same ring: one case of
each at a small ring, the latter against tests/framer_features_oracle.py."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
import clips
from viz_player_oracle import unit_chain

pytestmark = pytest.mark.gpu

KW = dict(tps=255 * 30, ref_interval=255, output_fps=30.0, codec_version=2)  # 255 ticks per output frame
K_ABS, K_DT = 16, 32  # the window depth for delta_t_max <= 12 * 255 (AbsoluteT) / delta_t_max = 255 (DeltaT)

#        name                  W   H  C  time mode     multi mode  dtm      clip     ring      value type
CASES = [
    ("one-unit-below-K", 1, 1, 1, O.ABSOLUTE_T, O.NORMAL, 255, "noise", 5, 0),
    ("35-units-at-K", 7, 5, 1, O.ABSOLUTE_T, O.NORMAL, 255, "noise", K_ABS, 0),  # a tile that is not full
    ("260-units-above-K", 20, 13, 1, O.ABSOLUTE_T, O.NORMAL, 255, "noise", K_ABS + 5, 0),  # a full tile and 4 units
    ("261-units-below-K", 9, 29, 1, O.ABSOLUTE_T, O.NORMAL, 255, "noise", 5, 0),  # a full tile, rows byte by byte
    ("512-units-above-K", 32, 16, 1, O.ABSOLUTE_T, O.NORMAL, 255, "noise", K_ABS + 5, 0),  # two full tiles, vector rows
    ("512-units-at-K", 32, 16, 1, O.ABSOLUTE_T, O.NORMAL, 255, "noise", K_ABS, 0),
    ("264-units-rgb-below-K", 11, 8, 3, O.ABSOLUTE_T, O.NORMAL, 255, "noise", 5, 0),
    ("36-units-rgb-above-K", 4, 3, 3, O.ABSOLUTE_T, O.NORMAL, 255, "noise", K_ABS + 5, 0),
    ("260-units-deltat-at-K", 20, 13, 1, O.DELTA_T, O.NORMAL, 255, "noise", K_DT, 0),
    ("35-units-deltat-above-K", 7, 5, 1, O.DELTA_T, O.NORMAL, 255, "noise", K_DT + 5, 0),
    ("512-units-deltat-below-K", 32, 16, 1, O.DELTA_T, O.NORMAL, 255, "noise", 5, 0),
    ("35-units-u16", 7, 5, 1, O.ABSOLUTE_T, O.NORMAL, 255, "noise", 5, 1),  # wider ring elements: the slot stride
    ("260-units-u32", 20, 13, 1, O.ABSOLUTE_T, O.NORMAL, 255, "noise", K_ABS + 5, 2),
    # Collapse: a pixel speaks when it changes; one that changes every fourth source frame holds the frames back
    ("260-units-collapse-below-K", 20, 13, 1, O.ABSOLUTE_T, O.COLLAPSE, 255 * 4, "noise", 12, 0),
    ("512-units-collapse-above-K", 32, 16, 1, O.ABSOLUTE_T, O.COLLAPSE, 255 * 4, "noise", K_ABS + 5, 0),
]


@functools.lru_cache(maxsize=None)
def build(name):
    """The reference side of a case, no GPU: events per source frame, the batches and what they reach.
    -> dict(per, batches [(k0, k1, w0, top)], ...)"""
    _, W, H, C, time_mode, multi_mode, dtm, kind, ring, vt = next(c for c in CASES if c[0] == name)
    T = 4 * ring + 3 + (2 * dtm // 255 if multi_mode == O.COLLAPSE else 0)
    clip = clips.make_clip(kind, T, H, W, C, seed=len(name) + ring)
    if multi_mode == O.COLLAPSE:  # a pixel that is silent for four source frames at a time
        clip[:, 0, 0, :] = np.random.default_rng(ring).integers(1, 256, T // 4 + 1).astype(np.uint8)[np.arange(T) // 4, None]
    ov = O.Video(W, H, C, time_mode=time_mode, multi_mode=multi_mode, delta_t_max=dtm)
    ov.ensure_capacity(26)
    ov.set_crf_parameters(0, 10)
    ov.reset_c_thresh(0)
    per = [ov.integrate_matrix(f).copy() for f in clip]
    ev = np.concatenate(per)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in per])])
    _, frm, to, _, unit = unit_chain(ev, W, C, tpf=255, ref_interval=255, abs_t=time_mode == O.ABSOLUTE_T, round_up=True)
    n_units = W * H * C
    top_of = [int(np.max(np.where(to[a:b] > frm[a:b], to[a:b], -1), initial=-1)) for a, b in zip(offs[:-1], offs[1:])]
    lastf = np.full(n_units, -1, np.int64)
    batches, k, j = [], 0, 0
    while k < T:
        w0 = int(lastf.min()) + 1  # frames_written once every complete frame is popped
        cap = ring if j % 2 == 0 else (j // 2) % (ring - 1) + 1
        n = 0
        while k + n < T and n < cap and top_of[k + n] < w0 + ring:
            n += 1
        assert n >= 1, (name, k, w0, top_of[k])  # the ring holds no single source frame here: choose another stream
        a, b = offs[k], offs[k + n]
        np.maximum.at(lastf, unit[a:b], to[a:b])
        batches.append((k, k + n, w0, max(top_of[k:k + n])))
        k, j = k + n, j + 1
    return dict(W=W, H=H, C=C, time_mode=time_mode, dtm=dtm, ring=ring, vt=vt, per=per, batches=batches,
                w_end=int(lastf.min()) + 1, held=int(lastf.max()) - int(lastf.min()),
                straddle=sum(1 for _, _, w0, top in batches if w0 % ring and w0 % ring + (top - w0 + 1) > ring),
                last_slot=sum(1 for _, _, w0, top in batches if top == w0 + ring - 1))


def run(name, path):
    """-> frames of the HIP framer, frames of the reference (both with the flush epilogue's frames appended)"""
    import torch
    import adder_amd as A
    c = build(name)
    W, H, C, ring, vt = c["W"], c["H"], c["C"], c["ring"], c["vt"]
    kw = dict(KW, delta_t_max=c["dtm"], time_mode=c["time_mode"])
    ofr = O.Framer(W, H, C, chunk_rows=64, source_camera=O.FRAMED_U8, **kw)
    if vt:
        ofr.set_view(0, vt, 0.0)
        ofr.set_value_type(vt)
    fr = A.HipFramer(W, H, C, source_camera=A.FRAMED_U8, ring_frames=ring, value_type=vt, source_type=vt, **kw)
    st_ = torch.cuda.current_stream().cuda_stream
    want = got = b""
    for k0, k1, w0, top in c["batches"]:
        assert fr.frames_written == w0 >= ofr.frames_written and top < w0 + ring
        segs = c["per"][k0:k1]
        ev = np.concatenate(segs)
        offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
        want += ofr.ingest_events(ev)
        if path == "batch":
            d_ev = torch.from_numpy(ev.view(np.uint8).copy()).cuda() if len(ev) else torch.zeros(12, dtype=torch.uint8, device="cuda")
            fr.ingest_frames_device(d_ev, offs, stream=st_)  # E_OUT_CAPACITY (the ring) raises: a failure
        else:
            fr.ingest(ev, offs)
        got += fr.pop()
        m = min(len(got), len(want))
        assert got[:m] == want[:m], (name, k0)
    assert got == want
    assert ofr.frames_written == fr.frames_written == c["w_end"] >= 3 * ring  # the ring wrapped three times
    flushed = []
    for _ in range(2):
        a, b = ofr.flush_frame_buffer(), fr.flush_frame_buffer()
        assert a == b
        flushed.append(a)
        x, y = ofr.write_frame_bytes(), fr.write_frame_bytes()
        assert x == y
        want, got = want + x, got + y
        assert ofr.frames_written == fr.frames_written
    fr.close()
    return got, want, flushed


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_batches_through_a_ring_that_wraps(name):
    c = build(name)
    assert len(c["per"]) >= 4 * c["ring"] and c["w_end"] >= 3 * c["ring"]
    assert c["straddle"] >= 2 and c["last_slot"] >= 2  # batches that pass the end of the ring / reach its last slot
    got, want, flushed = run(name, "batch")
    assert got == want
    if "collapse" in name:  # frames held back by the silent pixel, handed out by the flush from wrapped slots
        assert c["held"] >= 2 and flushed[0] and c["w_end"] % c["ring"] != 0


@pytest.mark.parametrize("name", ["260-units-above-K", "260-units-collapse-below-K"])
def test_the_segment_kernel_gives_the_same_frames_through_the_same_ring(name):
    got, want, _ = run(name, "segments")
    assert got == want and got == run(name, "batch")[0]


# ---- detection on: the feature pass fills the same ring --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def detection_case():
    """24 x 20 noise, three source frames per call -> params, ops, the restatement's log, the smallest ring, the
    frames_written in front of every call (from the events alone)"""
    import framer_features_cases as FK
    import framer_features_oracle as FR
    W, H, T, per_call = 24, 20, 36, 3
    clip = clips.make_clip("noise", T, H, W, 1, seed=5)
    frames = FR.transcode(clip, time_mode=O.ABSOLUTE_T, multi_mode=O.NORMAL, crf=0, delta_t_max=510)
    ev = np.concatenate(frames)
    offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    _, frm, to, _, unit = unit_chain(ev, W, 1, tpf=255, ref_interval=255, abs_t=True, round_up=True)
    lastf = np.full(W * H, -1, np.int64)
    need, starts, ops = 0, [], [("detect", True)]
    for k in range(0, T, per_call):
        a, b = offs[k], offs[min(k + per_call, T)]
        starts.append(int(lastf.min()) + 1)
        need = max(need, int(np.max(np.where(to[a:b] > frm[a:b], to[a:b], -1))) - starts[-1] + 1)
        np.maximum.at(lastf, unit[a:b], to[a:b])
        ops += [("ingest", ev[a:b]), ("pop_with_features", None)]
    params = dict(KW, delta_t_max=510, width=W, height=H, channels=1, time_mode=O.ABSOLUTE_T)
    return params, ops, FK.run(FR.Restatement(**params), ops), need, starts, int(lastf.min()) + 1


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("entry", ["frames", "device"])
def test_detection_fills_a_ring_that_wraps(entry, extra):
    """detect_features on (adder_framer_features.hip stores the frames' values itself, at f % ring_frames): features,
    popped frames, intervals and the running plane against the restatement, the ring at its smallest and one more"""
    import framer_features_cases as FK
    from test_gpu_framer_features import Dev
    params, ops, want, need, starts, w_end = detection_case()
    ring = need + extra
    assert ring <= 6 and w_end >= 4 * ring and sum(1 for w in starts if w % ring) >= 3
    assert sum(len(f) for f in want["features"]) >= 100
    got = FK.run(Dev(dict(params, ring_frames=ring), entry), ops)
    assert got["features"] == want["features"]
    assert got["frames"] == want["frames"] and len(b"".join(got["frames"])) == w_end * 24 * 20
    assert got["pops"] == want["pops"]
    assert np.array_equal(got["plane"], want["plane"])
