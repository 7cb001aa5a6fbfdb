"""The packed frame kernel (adder_lp_kernel) and its expansion (adder_lpx_kernel<9 | 11 | 12>) at their edges: row
lengths on both sides of every threshold of the expansion's coordinate decode, escape words (rho' >= 255) of every rank,
destination buffers at every byte phase, capacities that end inside the stream.  Everything is DeltaT, Collapse,
delta_t_max = ref_time = 255, c_thresh 0 (the packed kernel's regime), goes through BOTH outputs -- AdderEvents
(integrate_device, 12 bytes) and the raw sink's records (integrate_wire_device, 9 / 11 bytes) -- and is compared byte for
byte with the oracle; every output buffer has 64 bytes of 0xAB in front and behind, which must survive.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import clips

GUARD = 64
FILL = 0xAB


def _hip():
    import adder_amd
    return adder_amd


def _oracle(W, rows, Cn, row_begin=0, time_mode=O.DELTA_T, multi_mode=O.COLLAPSE, dtm=255):
    ov = O.Video(W, rows, Cn, row_begin=row_begin, time_mode=time_mode, multi_mode=multi_mode, ref_time=255, delta_t_max=dtm)
    ov.ensure_capacity(24)
    ov.set_crf_parameters(0, 10)
    ov.reset_c_thresh(0)
    return ov


def _video(W, H, Cn, band=None, time_mode=O.DELTA_T, multi_mode=O.COLLAPSE, dtm=255):
    A = _hip()
    y0, y1 = (0, H) if band is None else band
    hv = A.HipVideo(W, H, Cn, row_begin=y0, row_end=y1, time_mode=time_mode, multi_mode=multi_mode, ref_time=255,
                    delta_t_max=dtm, max_depth=24, c_thresh_start=0, c_counter_start=0)  # (what reset() goes back to)
    hv.set_crf_parameters(0, 10)
    hv.reset_c_thresh(0)
    return hv


def _want(clip, band=None, **mode):
    """The oracle's events of every frame of clip [T][H][W][C] (of the rows of `band`)."""
    _, H, W, Cn = clip.shape
    y0, y1 = (0, H) if band is None else band
    ov = _oracle(W, y1 - y0, Cn, row_begin=y0, **mode)
    return [ov.integrate_matrix(f) for f in clip[:, y0:y1]]


def _rec(form, Cn):
    return 12 if form == "events" else (9 if Cn == 1 else 11)


def _bytes(per, form, Cn):
    ev = np.concatenate(per) if len(per) else np.zeros(0, O.EVENT_DTYPE)
    return ev.tobytes() if form == "events" else O.raw_events(ev, Cn)


def _units(ev, W, Cn, row_begin=0):
    """Unit index (raster order of the band, channels interleaved) of every event."""
    c = np.where(ev["c"] == 0xFF, 0, ev["c"]).astype(np.int64)
    return ((ev["y"].astype(np.int64) - row_begin) * W + ev["x"]) * Cn + c


class _Guarded:
    """An output buffer of `nbytes` at byte phase `phase` (mod 16) with GUARD bytes of FILL in front (the `phase` bytes that
    share its first 16-byte block included) and behind."""

    def __init__(self, nbytes, phase=0):
        import torch
        self.lo, self.n = GUARD + phase, nbytes
        self.big = torch.full((self.lo + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert self.big.data_ptr() % 16 == 0
        self.out = self.big[self.lo:self.lo + nbytes]
        assert self.out.numel() == nbytes and (nbytes == 0 or self.out.data_ptr() % 16 == phase % 16)

    def check(self, want, tag, written=None):
        """Guards intact; the first `written` (default: all) bytes equal `want`, the rest of the buffer is still FILL."""
        host = self.big.cpu().numpy()
        written = self.n if written is None else written
        assert (host[:self.lo] == FILL).all(), ("bytes in front of the buffer", tag)
        assert (host[self.lo + written:] == FILL).all(), ("bytes behind the stream", tag)
        assert host[self.lo:self.lo + written].tobytes() == want[:written], tag


def _submit(hv, form, d_frames, out, d_offs, st):
    if form == "events":
        hv.integrate_device(d_frames, out, d_offs, stream=st)
    else:
        hv.integrate_wire_device(d_frames, out, d_offs, stream=st)


def _run(hv, clip_rows, want, batches, form, tag, phase=0, packed=True):
    """clip_rows [T][rows][W][C] through hv in `batches`, every batch into a guarded buffer of exactly its size at `phase`."""
    import torch
    A = _hip()
    st = torch.cuda.current_stream().cuda_stream
    Cn = clip_rows.shape[3]
    rec = _rec(form, Cn)
    k = 0
    for nb in batches:
        per = want[k:k + nb]
        n = sum(len(p) for p in per)
        d_frames = torch.from_numpy(np.ascontiguousarray(clip_rows[k:k + nb]).reshape(nb, -1)).cuda()
        buf = _Guarded(n * rec, phase)
        d_offs = torch.full((nb + 1,), -1, dtype=torch.int64, device="cuda")
        _submit(hv, form, d_frames, buf.out, d_offs, st)
        assert hv.finish() == n, (tag, form, k, nb)
        if nb > 1 and packed:
            assert hv.last_batch_kernel() == A.KERNEL_LEAN_RUNS_PACKED, (tag, form, k, nb, hv.last_batch_kernel())
        assert d_offs.cpu().tolist() == np.concatenate([[0], np.cumsum([len(p) for p in per])]).tolist(), (tag, form, k, nb)
        buf.check(_bytes(per, form, Cn), (tag, form, k, nb, phase))
        k += nb
    assert k == len(clip_rows)


# ---- 1. row lengths ---------------------------------------------------------------------------------------------
PLANES = [
    # 1024 <= rowlen < 2048: a wave's units span up to three rows
    (341, 7, 3, None), (1024, 7, 1, None), (1025, 7, 1, None), (342, 7, 3, None), (2047, 4, 1, None),
    # rowlen >= 2048: up to two rows
    (2048, 4, 1, None), (2049, 4, 1, None), (683, 4, 3, None), (4097, 2, 1, None),
    # the divide path: one wave over many rows
    (1, 4100, 1, None), (1, 1400, 3, None), (7, 600, 1, None), (127, 40, 1, None), (128, 40, 1, None), (129, 40, 1, None),
    (255, 20, 1, None), (257, 20, 1, None), (1000, 7, 1, None),
    # a row band: row_begin > 0
    (1025, 12, 1, (5, 12)), (683, 9, 3, (3, 9)),
]


def _row_clip(kind, W, H, Cn, band, seed):
    """(clip, batches): 40 frames as 2, 1, 37.  `steps` gets four frames more -- copies of the frame in front of them, so
    that frames without a single event occur inside and at the end of a batch -- and keeps the units of the band's first
    wave (and the quarter of a wave behind it) still from frame 20 on, so that busy frames have a wave without an event."""
    clip = clips.make_clip(kind, 40, H, W, Cn, seed=seed)
    if kind != "steps":
        return clip, (2, 1, 37)
    y0, y1 = (0, H) if band is None else band
    rows_still = -(-(2048 + 512) // (W * Cn))
    clip[20:, y0:y0 + rows_still] = clip[19, y0:y0 + rows_still]
    clip = np.concatenate([clip[:1], clip[:1], clip[1:21], clip[20:21], clip[20:21], clip[21:], clip[-1:]])
    return clip, (2, 1, 37, 4)


@pytest.mark.parametrize("W,H,Cn,band", PLANES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_row_lengths(W, H, Cn, band):
    y0, y1 = (0, H) if band is None else band
    n_units = W * (y1 - y0) * Cn
    assert n_units > 2 * 2048  # more than two of the expansion's waves: the third starts inside a row
    for kind in ("runs", "noise", "steps"):
        clip, batches = _row_clip(kind, W, H, Cn, band, seed=W * 7 + H + Cn)
        want = _want(clip, band)
        per_pair = [np.bincount(_units(e, W, Cn, y0) // 256, minlength=-(-n_units // 256)) for e in want]
        if kind == "noise":  # dense: a frame in which a 256-unit pair emits more than 64 events (nearly all do)
            assert any(p.max() > 64 for p in per_pair)
        if kind == "steps":  # whole frames without an event, and busy frames whose first wave (8 pairs) has none
            assert any(len(e) == 0 for e in want[1:])
            assert any(p.sum() > 0 and p[:8].sum() == 0 for p in per_pair)
        for form in ("events", "wire"):
            hv = _video(W, H, Cn, band)
            _run(hv, clip[:, y0:y1], want, batches, form, (W, H, Cn, band, kind))
            hv.close()


# ---- 2. escape words --------------------------------------------------------------------------------------------
def _escape_clip(W, Cn, staggered=False):
    """300 frames of a still random plane of three rows; unit u of rows 0 and 2 flips at frame 250 + u % 12, every unit of
    row 1 at frame 270.  `staggered`: unit u of row 1 also changes once before, at frame 1 + u % 7 -- its run at frame 270 is
    263..269 frames by the unit, so the pair's 256 escape words differ, and differ between its rounds of 64 records (an
    escape word holds the run length and nothing else: equal runs make every escape slot read the same)."""
    rng = np.random.default_rng(W * 10 + Cn)
    T, H = 300, 3
    base = rng.integers(1, 256, (H, W, Cn), dtype=np.uint8)
    clip = np.broadcast_to(base, (T, H, W, Cn)).copy()
    flat = clip.reshape(T, H, W * Cn)
    for row in (0, 2):
        for j in range(W * Cn):
            u = row * W * Cn + j
            flat[250 + u % 12:, row, j] = 255 - flat[0, row, j]
    if staggered:
        for j in range(W * Cn):
            u = W * Cn + j
            flat[1 + u % 7:, 1, j] = 1 + (int(flat[0, 1, j]) + 50) % 255  # (another non-zero value)
    flat[270:, 1, :] = 255 - flat[269, 1, :]
    return clip


def _escape_runs(clip):
    """Per frame: (unit, frames since the unit's value last changed) of every unit that changes in it -- from the clip alone."""
    flat = clip.reshape(len(clip), -1).astype(np.int64)
    last = np.zeros(flat.shape[1], np.int64)
    out = []
    for f in range(1, len(flat)):
        ch = np.nonzero(flat[f] != flat[f - 1])[0]
        out.append((f, ch, f - last[ch]))
        last[ch] = f
    return out


@pytest.mark.parametrize("staggered", [False, True], ids=["equal_runs", "staggered"])
@pytest.mark.parametrize("W,Cn", [(256, 1), (86, 3)])
def test_escape_words(W, Cn, staggered):
    """Runs of 250..261 frames (rho' on both sides of 254 / 255 / 256), a frame in which a pair's every record escapes, frames
    whose escaping records lie behind the pair's first round of 64 -- as one launch sequence of 300 frames and as batches
    that carry the runs from launch to launch.  (On 86 x 3 a row is 258 units, so row 1 fills all of pair 1 but its first
    two units: 254 escapes in one pair.)  `staggered`: the escaping records of that pair have different run lengths at the
    same rank of different rounds of 64, so an escape word read at the wrong rank (the rank counts the rounds before) shows
    in the events' t; with equal runs it could not."""
    clip = _escape_clip(W, Cn, staggered)
    runs = _escape_runs(clip)
    lengths = np.concatenate([r for _, _, r in runs])
    assert set(range(250, 262)) <= set(lengths.tolist())
    long_per_pair = [(f, np.bincount(u[r >= 256] // 256, minlength=4), u[r >= 256] % 256) for f, u, r in runs]
    n_full = 256 if W * Cn == 256 else 254
    full = [f for f, cnt, _ in long_per_pair if cnt.max() == n_full]
    assert full == [270]
    assert any(f != 270 and cnt.max() > 0 and (pos >= 64).any() for f, cnt, pos in long_per_pair)
    # frame 270, pair 1: every record escapes; record k of the pair (unit order) belongs to round k // 64 and has rank k
    u270, r270 = next((u, r) for f, u, r in runs if f == 270)
    pair_runs = r270[u270 // 256 == 1]
    assert len(pair_runs) == n_full and (pair_runs >= 256).all()
    if staggered:
        for k in range(1, -(-n_full // 64)):  # the same place in another round: always another run length
            later = pair_runs[64 * k:64 * k + 64]
            assert (later != pair_runs[:len(later)]).all() and (later != pair_runs[64 * (k - 1):64 * (k - 1) + len(later)]).all()
    else:
        assert (pair_runs == 270).all()
    want = _want(clip)
    for batches in ((300,), (64, 64, 64, 64, 44)):
        for form in ("events", "wire"):
            hv = _video(W, 3, Cn)
            _run(hv, clip, want, batches, form, (W, Cn, batches))
            hv.close()


# ---- 3. destination phase ---------------------------------------------------------------------------------------
OTHER_WIRE_FORMATS = [(O.ABSOLUTE_T, O.COLLAPSE, 255), (O.DELTA_T, O.COLLAPSE, 7650), (O.DELTA_T, O.NORMAL, 255)]


@functools.lru_cache(maxsize=None)
def _phase_case(Cn, mode=(O.DELTA_T, O.COLLAPSE, 255)):
    clip = clips.make_clip("runs", 13, 61, 157, Cn, seed=31 + Cn)
    # the last three frames: still, but for the plane's last unit, which takes a new non-zero value in each -- the last frame's
    # only event is ONE record (9 / 11 / 12 bytes: less than a 16-byte block) at the very end of the stream
    clip[10:] = clip[9]
    for k in (10, 11, 12):
        clip[k, -1, -1, -1] = 1 + (int(clip[k - 1, -1, -1, -1]) + 50) % 255
    tm, mm, dtm = mode
    want = _want(clip, time_mode=tm, multi_mode=mm, dtm=dtm)
    assert mode != (O.DELTA_T, O.COLLAPSE, 255) or len(want[-1]) == 1
    return clip, want


PHASE_BATCHES = (2, 1, 4, 3, 3)  # (a single frame plans the per-frame record forms; the last batch ends in the one-record frame)


@pytest.mark.parametrize("Cn", [1, 3])
def test_destination_phase_packed(Cn):
    """The contract (include/adder_hip.h): d_wire at ANY byte address, AdderEvents at any multiple of 4.  The expansion
    stages at the 16-byte phase of its destination and writes the <= 15 bytes in front of its first whole block singly: the
    `p` bytes between the 16-byte boundary and the buffer are the neighbour's."""
    clip, want = _phase_case(Cn)
    hv = _video(157, 61, Cn)
    for form, phases in (("wire", range(16)), ("events", (0, 4, 8, 12))):
        for p in phases:
            hv.reset()
            _run(hv, clip, want, PHASE_BATCHES, form, ("phase", Cn), phase=p)
    hv.close()


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("mode", OTHER_WIRE_FORMATS, ids=["abs_t", "bounded", "normal"])
def test_destination_phase_other_wire_formats(Cn, mode):
    """The same entry point when the plan picks another expansion (lean AbsoluteT, run records / bounded Collapse, generic
    Normal): one rule for all of them -- any byte address."""
    clip, want = _phase_case(Cn, mode)
    tm, mm, dtm = mode
    hv = _video(157, 61, Cn, time_mode=tm, multi_mode=mm, dtm=dtm)
    for p in range(16):
        hv.reset()
        _run(hv, clip, want, PHASE_BATCHES, "wire", ("phase", Cn, mode), phase=p, packed=False)
    hv.close()


@pytest.mark.parametrize("Cn", [1, 3])
def test_wire_events_device_at_every_phase(Cn):
    """adder_hip_wire_events_device (AdderEvents in HBM -> wire records) into a buffer at every byte phase."""
    import torch
    clip, want = _phase_case(Cn)
    ev = np.concatenate(want)[:3001]  # (more than two workgroups of 1024 events, the last one ragged)
    rec = 9 if Cn == 1 else 11
    hv = _video(157, 61, Cn)
    d_ev = torch.from_numpy(ev.view(np.uint8).copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for p in range(16):
        buf = _Guarded(len(ev) * rec, p)
        assert hv.wire_events_device(d_ev, len(ev), buf.out, stream=st) == len(ev) * rec
        torch.cuda.synchronize()
        buf.check(O.raw_events(ev, Cn), ("wire_events", Cn, p))
    hv.close()


def test_misaligned_event_source_is_refused():
    """adder_hip_wire_events_device reads AdderEvents as dwords: a d_events that is no multiple of 4 is refused -- BAD_PARAMS,
    last_error set, nothing written -- and the context converts the same events afterwards."""
    import torch
    A = _hip()
    clip, want = _phase_case(1)
    ev = np.concatenate(want)[:1500]
    hv = _video(157, 61, 1)
    st = torch.cuda.current_stream().cuda_stream
    raw = torch.from_numpy(ev.view(np.uint8).copy()).cuda()
    for p in (1, 2, 3):
        shifted = torch.zeros(raw.numel() + 16, dtype=torch.uint8, device="cuda")
        shifted[p:p + raw.numel()] = raw
        d_ev = shifted[p:p + raw.numel()]
        assert d_ev.data_ptr() % 4 == p
        buf = _Guarded(len(ev) * 9)
        with pytest.raises(A.AdderHipError) as ei:
            hv.wire_events_device(d_ev, len(ev), buf.out, stream=st)
        assert ei.value.code == A.E_BAD_PARAMS and "align" in str(ei.value)
        assert b"align" in hv.L.adder_hip_last_error(hv.h)
        torch.cuda.synchronize()
        buf.check(b"", ("refused source", p), written=0)
    buf = _Guarded(len(ev) * 9, 5)
    assert hv.wire_events_device(raw, len(ev), buf.out, stream=st) == len(ev) * 9
    torch.cuda.synchronize()
    buf.check(O.raw_events(ev, 1), "after the refusals")
    hv.close()


def test_misaligned_event_buffer_is_refused():
    """AdderEvents are written as dwords: a d_out that is no multiple of 4 is refused before anything is queued -- BAD_PARAMS,
    the buffer untouched, and the context goes on as if the call had not been made."""
    import torch
    A = _hip()
    clip, want = _phase_case(1)
    hv = _video(157, 61, 1)
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.from_numpy(np.ascontiguousarray(clip[:2]).reshape(2, -1)).cuda()
    n = len(want[0]) + len(want[1])
    for p in (1, 2, 3, 7):
        buf = _Guarded(n * 12, p)
        d_offs = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        with pytest.raises(A.AdderHipError) as ei:
            hv.integrate_device(d_frames, buf.out, d_offs, stream=st)
        assert ei.value.code == A.E_BAD_PARAMS and "align" in str(ei.value)
        torch.cuda.synchronize()
        buf.check(b"", ("refused", p), written=0)
        assert d_offs.cpu().tolist() == [-1, -1, -1]
        with pytest.raises(A.AdderHipError):  # nothing is pending
            hv.finish()
    _run(hv, clip, want, PHASE_BATCHES, "events", "after the refusals")  # the stream starts at its first frame
    hv.close()


# ---- 4. capacity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 3])
def test_capacity_ends_inside_the_stream(Cn):
    """A 12-frame noise batch (every pair dense) into buffers that end inside the stream: E_OUT_CAPACITY with the size needed,
    the oracle's prefix in front of the capacity, not a byte behind it, and the retry -- then the next batch -- as if nothing
    had happened."""
    import torch
    A = _hip()
    W, H = 300, 9
    clip = clips.make_clip("noise", 16, H, W, Cn, seed=77 + Cn)
    want = _want(clip)
    per = want[:12]
    n = sum(len(p) for p in per)
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.from_numpy(np.ascontiguousarray(clip[:12]).reshape(12, -1)).cuda()
    for form in ("events", "wire"):
        rec = _rec(form, Cn)
        stream = _bytes(per, form, Cn)
        caps = [n * rec, (n - 1) * rec, (n - 17) * rec, (len(per[0]) + 3) * rec, 0]  # in bytes
        if form == "wire":
            caps.append(n * rec - 1)
        for cap_bytes in caps:
            hv = _video(W, H, Cn)
            cap = cap_bytes // rec  # in events
            buf = _Guarded(n * rec)  # (all of it FILL: what lies behind the capacity handed over is watched too)
            d_offs = torch.zeros(13, dtype=torch.int64, device="cuda")
            _submit(hv, form, d_frames, buf.out[:cap_bytes], d_offs, st)
            if cap == n:
                assert hv.finish() == n
                assert hv.last_batch_kernel() == A.KERNEL_LEAN_RUNS_PACKED
                buf.check(stream, (form, cap_bytes))
            else:
                with pytest.raises(A.AdderHipError) as ei:
                    hv.finish()
                assert hv.last_batch_kernel() == A.KERNEL_LEAN_RUNS_PACKED  # (the batch that overflowed ran the packed pair)
                assert ei.value.code == A.E_OUT_CAPACITY and hv.last_required == n, (form, cap_bytes, hv.last_required)
                buf.check(stream, (form, cap_bytes), written=cap * rec)
                _run(hv, clip[:12], per, (12,), form, ("retry", form, cap_bytes))
            # the next batch continues the stream
            _run(hv, clip[12:], want[12:], (4,), form, ("next", form, cap_bytes))
            hv.close()
