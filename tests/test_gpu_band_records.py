"""The band records hand-off and the root's expansion at their edges (include/adder_hip.h: adder_hip_integrate_records_device,
adder_hip_expand_records_device / _wire_device, adder_hip_records_to_wire; csrc/adder_kernels.hip: adder_slot_pack_kernel,
adder_log_bases_kernel, adder_log_pack_kernel, adder_band_layout_kernel, adder_expand_bands_kernel; host side:
csrc/adder_hip_records_api.cpp).  The cases are tests/band_records_cases.py's (tests/test_band_records_cpu.py shows on
the CPU that each reaches its edge): one context per band, every chunk integrated by every band and expanded by band 0
into one growing buffer.  The expected output is the oracle's events of the whole plane -- AdderEvents, or the raw sink's
9 / 11-byte records (oracle.raw_events) -- and the cumulative per-frame counts; everything is compared byte for byte.
Every output lies between 64 bytes of 0xAB, which must survive, as must whatever of the buffer the call may not write.

What no other GPU test runs, and the test here that does:
  more than kMaxBands bands (one launch per band)     test_merged_stream_equals_the_oracle[one_row_bands_17-*]
  adder_log_bases_kernel past its first trip          test_merged_stream_equals_the_oracle[segments_1040-*] (and _1024)
  multi-band log records expanded to AdderEvents      test_merged_stream_equals_the_oracle[*-log-events]
  a one-frame batch (log records without the switch)  test_merged_stream_equals_the_oracle[narrow_uneven | wide_uneven | rgb-*-runs-*]
  the wire expansion called directly: merged_base at  test_wire_output_at_every_byte_phase, test_capacity_ends_inside_the_stream
  a byte phase, too small a capacity, guard bytes
  the description block ring and its growth           test_description_blocks_are_reused_and_grow
  the wire image with several bands, a band without   test_wire_image_of_several_bands
  records, the image's own frame table, wire_sections
  every refusal, a root that never integrated         test_refusals_leave_the_root_usable
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import band_records_cases as BC

GUARD = 64
FILL = 0xAB
RUNS = 0x100  # ADDER_RECORDS_RUNS (include/adder_hip.h)


def _hip():
    import adder_amd
    return adder_amd


def _rec(form, Cn):
    return 12 if form == "events" else (9 if Cn == 1 else 11)


def _bytes(per, form, Cn):
    ev = np.concatenate(per) if len(per) else np.zeros(0, O.EVENT_DTYPE)
    return ev.tobytes() if form == "events" else O.raw_events(ev, Cn)


def _offsets(per, base=0):
    return np.cumsum([base] + [len(e) for e in per]).astype(np.int64)


class _Guarded:
    """A device buffer of `nbytes` (16-byte aligned) with GUARD bytes of FILL in front and behind, itself filled with FILL."""

    def __init__(self, nbytes):
        import torch
        self.n = nbytes
        self.big = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert self.big.data_ptr() % 16 == 0
        self.out = self.big[GUARD:GUARD + nbytes]

    def check(self, want, tag, first=0, written=None):
        """Guards intact; bytes [first, written) equal want[first:written]; the rest of the buffer is still FILL."""
        host = self.big.cpu().numpy()
        written = self.n if written is None else written
        assert (host[:GUARD + first] == FILL).all(), ("bytes in front of the stream", tag)
        assert (host[GUARD + written:] == FILL).all(), ("bytes behind the stream", tag)
        assert host[GUARD + first:GUARD + written].tobytes() == want[first:written], tag


class _Offsets:
    """An int64 offsets table of n entries between two guard entries."""
    MARK = -0x0123456789ABCDEF

    def __init__(self, n):
        import torch
        self.big = torch.full((n + 2,), self.MARK, dtype=torch.int64, device="cuda")
        self.out = self.big[1:n + 1]

    def check(self, want, tag):
        host = self.big.cpu().numpy()
        assert host[0] == self.MARK and host[-1] == self.MARK, ("offsets' guards", tag)
        assert np.array_equal(host[1:-1], want), ("offsets", tag)


# ---- the bands' contexts: those of ONE (case, time mode) at a time, reset() between tests ----
_live = {"key": None}


def _close_live():
    for hv in _live.get("ctxs", []):
        hv.close()
    _live.clear()
    _live["key"] = None


def _band_ctx(c, band):
    A = _hip()
    hv = A.HipVideo(c["W"], c["H"], c["Cn"], row_begin=band[0], row_end=band[1], time_mode=c["time_mode"], **BC.KW)
    hv.set_crf_parameters(*BC.CRF)
    return hv


def _bands_of(c, fresh=False):
    """(contexts, device frames [T][band units]) per band of the case, in the freshly constructed state."""
    import torch
    key = (c["name"], c["time_mode"])
    if _live["key"] != key or fresh:
        _close_live()
        _live["key"] = key
        _live["ctxs"] = [_band_ctx(c, b) for b in c["bands"]]
        T = c["clip"].shape[0]
        _live["frames"] = [torch.from_numpy(np.array(c["clip"][:, y0:y1]).reshape(T, -1)).cuda()
                           for y0, y1 in c["bands"]]
        _live["boffs"] = [torch.zeros(BC.MAX_CHUNK + 1, dtype=torch.int64, device="cuda") for _ in c["bands"]]
    else:
        for hv in _live["ctxs"]:
            hv.reset()
    return _live["ctxs"], _live["frames"]


@pytest.fixture(scope="module", autouse=True)
def _contexts_closed_at_the_end():
    yield
    _close_live()


# Everything -- the fills of the guarded buffers, the batches, the copies, the expansions -- is queued on ONE stream of the
# test's own: the contexts' streams do not wait for torch's default stream, so a buffer filled there could be filled
# after the expansion has written it.
_side = {}


@pytest.fixture(autouse=True)
def _on_one_stream():
    import torch
    if "stream" not in _side:
        _side["stream"] = torch.cuda.Stream()
    with torch.cuda.stream(_side["stream"]):
        yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device error is sticky: nothing after it in this process would mean anything
        pytest.exit(f"the device reported an error, the run ends here: {e}", returncode=3)


def _stream():
    import torch
    handle = torch.cuda.current_stream().cuda_stream
    assert handle != 0 and handle == _side["stream"].cuda_stream
    return handle


def _integrate_chunk(c, ctxs, frames, f0, nf, want_runs):
    """Every band integrates frames [f0, f0 + nf) and finishes; returns the descriptions and the records per band."""
    st = _stream()
    recs, n_records = [], []
    for r, hv in enumerate(ctxs):
        rec = hv.integrate_records_device(frames[r][f0:f0 + nf], _live["boffs"][r], stream=st)
        hv.finish()
        assert rec.num_frames == nf and rec.rows == c["bands"][r][1] - c["bands"][r][0] and rec.row_begin == c["bands"][r][0]
        assert rec.num_segments == hv.band_segments() == c["segments"][r], (r, rec.num_segments)
        assert bool(rec.record_bytes & RUNS) == want_runs, ("record kind", r, f0, nf)
        assert rec.record_bytes & 0xff == (12 if c["time_mode"] == BC.ABSOLUTE_T else 8)
        recs.append(rec)
        n_records.append(hv.last_batch_records())
    return recs, n_records


def _expand(root, form, recs, out, merged_base, d_moff):
    if form == "events":
        root.expand_records_device(recs, out, merged_base, d_moff, stream=_stream())
    else:
        root.expand_records_wire_device(recs, out, merged_base, d_moff, stream=_stream())


def _run_case(c, kind, form, merged_base=0, chunks=None):
    """The common driver: every chunk through every band, band 0 expands into one growing buffer at merged_base."""
    ctxs, frames = _bands_of(c)
    per = BC.oracle_events(c["name"], c["time_mode"])
    rec = _rec(form, c["Cn"])
    want = bytes([FILL]) * (merged_base * rec) + _bytes(per, form, c["Cn"])
    want_off = _offsets(per, merged_base)
    buf = _Guarded(len(want))
    moff = _Offsets(len(per) + 1)
    f0, kinds = 0, []
    for nf in (c["chunks"] if chunks is None else chunks):
        want_runs = kind == "runs" and nf > 1  # (plan_batch: the lean-runs kernel takes batches of two frames and more)
        recs, _ = _integrate_chunk(c, ctxs, frames, f0, nf, want_runs)
        _expand(ctxs[0], form, recs, buf.out, int(want_off[f0]), moff.out[f0:])
        ctxs[0].expand_status(stream=_stream())
        kinds.append(want_runs)
        f0 += nf
    assert f0 == len(per)
    tag = (c["name"], BC.TIME_IDS[c["time_mode"]], kind, form, merged_base)
    moff.check(want_off, tag)
    buf.check(want, tag, first=merged_base * rec)
    return kinds


def _grid():
    out = []
    for name in BC.NAMES:
        for tm in BC.TIME_MODES:
            # (the two segments_* cases are there for adder_log_bases_kernel: the log kind alone)
            for kind in (("log",) if name.startswith("segments_") else ("runs", "log")):
                for form in ("events", "wire"):
                    out.append(pytest.param(name, tm, kind, form, id=f"{name}-{BC.TIME_IDS[tm]}-{kind}-{form}"))
    return out


# ---- 1: every case x time mode x record kind x output form ----
@pytest.mark.parametrize("name,time_mode,kind,form", _grid())
def test_merged_stream_equals_the_oracle(monkeypatch, name, time_mode, kind, form):
    if kind == "log":
        monkeypatch.setenv("ADDER_HIP_NO_LR", "1")
    c = BC.case(name, time_mode)
    if name in BC.SEGMENTS:
        assert c["segments"] == BC.SEGMENTS[name]
    kinds = _run_case(c, kind, form)
    if kind == "runs" and 1 in c["chunks"]:  # the one-frame chunk came out as log records, its neighbours as runs
        assert kinds == [nf > 1 for nf in c["chunks"]] and not all(kinds) and any(kinds)


@pytest.mark.parametrize("time_mode", BC.TIME_MODES, ids=BC.TIME_IDS.get)
def test_whole_plane_context_agrees_with_the_oracle(time_mode):
    """The other reference of test_gpu_records.py: one context over the whole plane (adder_hip_integrate_device)."""
    import torch
    A = _hip()
    c = BC.case("narrow_uneven", time_mode)
    per = BC.oracle_events(c["name"], time_mode)
    T = c["clip"].shape[0]
    hv = A.HipVideo(c["W"], c["H"], c["Cn"], time_mode=time_mode, **BC.KW)
    hv.set_crf_parameters(*BC.CRF)
    d_all = torch.from_numpy(np.array(c["clip"]).reshape(T, -1)).cuda()  # (a copy: the case's clip is read-only)
    n_want = sum(len(e) for e in per)
    d_ev = torch.empty((n_want + 16, 3), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv.integrate_device(d_all, d_ev, d_off, stream=_stream())
    assert hv.finish() == n_want
    assert d_ev[:n_want].cpu().numpy().tobytes() == _bytes(per, "events", c["Cn"])
    assert np.array_equal(d_off.cpu().numpy(), _offsets(per))
    hv.close()


# ---- 2: the records per segment the expansion's two paths are chosen by ----
def _image_of(hv, rec, n_records, short=0):
    """adder_hip_records_to_wire of the band's last batch into a guarded buffer (`short` bytes too small)."""
    from adder_amd import records as R
    nbytes = R.wire_bytes(rec.num_frames, rec.num_segments, rec.record_bytes, n_records)
    img = _Guarded(nbytes - short)
    hv.records_to_wire(rec, n_records, img.out, stream=_stream())
    return img


@pytest.mark.parametrize("kind", ["runs", "log"])
def test_records_per_segment_reach_both_expansion_paths(monkeypatch, kind, capsys):
    """narrow_uneven's d_counts ([nf][num_segments], records in the high half), copied back through the wire image: (segment,
    frame) pairs without a record, with 1 .. 32 (expanded as a pair of segments) and with more (one segment at a time)."""
    import torch
    from adder_amd import records as R
    if kind == "log":
        monkeypatch.setenv("ADDER_HIP_NO_LR", "1")
    c = BC.case("narrow_uneven", BC.DELTA_T)
    ctxs, frames = _bands_of(c)
    seen, as_changed = [set() for _ in ctxs], []
    f0 = 0
    for nf in c["chunks"]:
        recs, n_records = _integrate_chunk(c, ctxs, frames, f0, nf, kind == "runs" and nf > 1)
        for r, hv in enumerate(ctxs):
            img = _image_of(hv, recs[r], n_records[r])
            torch.cuda.synchronize()
            sec = R.wire_sections(nf, recs[r].num_segments, recs[r].record_bytes)
            counts = img.out[sec[2]:sec[2] + nf * recs[r].num_segments * 4].cpu().numpy().view(np.uint32)
            per_seg = (counts >> 16).reshape(nf, recs[r].num_segments)
            assert int(per_seg.sum()) == n_records[r]
            seen[r] |= set(np.unique(per_seg).tolist())
            if f0 > 0:  # (frames after the first: the generator's changed units, test_band_records_cpu.py)
                changed = BC.changed_units(c, r)[f0 - 1:f0 - 1 + nf]
                as_changed.append(bool(np.array_equal(per_seg[:, :changed.shape[1]], changed)))
        f0 += nf
    with capsys.disabled():  # (the census band_records_cases.py's docstring records)
        print(f"\n[census] narrow_uneven {kind}: records == units changed in {sum(as_changed)} of {len(as_changed)} (band, chunk) "
              f"pairs after the first chunk; records per (segment, frame) seen per band: "
              f"{[(min(s), max(s), len(s), sorted(s & {0, 1, 32, 33, BC.WAVE_UNITS})) for s in seen]} as (min, max, distinct, of the census)")
    every = set().union(*seen)
    assert 0 in every and any(1 <= v <= 32 for v in every) and any(v > 32 for v in every)
    assert {0, 1, 32, 33} <= every and max(every) == BC.WAVE_UNITS


# ---- 3: wire output at every byte phase ----
@pytest.mark.parametrize("merged_base", [0, 1, 2, 3])
@pytest.mark.parametrize("name,time_mode,kind", [("rowlen_255", BC.DELTA_T, "runs"), ("rowlen_255", BC.ABSOLUTE_T, "log"),
                                                  ("rgb", BC.ABSOLUTE_T, "runs"), ("rgb", BC.DELTA_T, "log")])
def test_wire_output_at_every_byte_phase(monkeypatch, name, time_mode, kind, merged_base):
    """adder_hip_expand_records_wire_device with the merged stream starting at event 0 .. 3 of the buffer: every phase of a
    9-byte and of an 11-byte record against the dwords the expansion stores; the bytes in front stay, offsets[0] ==
    merged_base (_run_case checks both)."""
    if kind == "log":
        monkeypatch.setenv("ADDER_HIP_NO_LR", "1")
    _run_case(BC.case(name, time_mode), kind, "wire", merged_base=merged_base)


# ---- 4: capacity ----
def _band_index(c, ev):
    return np.searchsorted(np.array([b[1] for b in c["bands"]]), ev["y"], side="right")


@pytest.mark.parametrize("form", ["events", "wire"])
@pytest.mark.parametrize("name,time_mode", [("rowlen_256", BC.DELTA_T), ("rgb", BC.ABSOLUTE_T)])
def test_capacity_ends_inside_the_stream(name, time_mode, form):
    """The first chunk into buffers too small: one event short, ending inside a band's share of a frame and (wire) at a byte
    that is no record's end.  ADDER_E_OUT_CAPACITY, nothing at or past the capacity written, the events in front of it are
    the stream's, the offsets the full ones; the same root then expands the same descriptions into a buffer that fits."""
    A = _hip()
    c = BC.case(name, time_mode)
    ctxs, frames = _bands_of(c)
    nf = c["chunks"][0]
    per = BC.oracle_events(name, time_mode)[:nf]
    rec = _rec(form, c["Cn"])
    want, want_off = _bytes(per, form, c["Cn"]), _offsets(per)
    total = int(want_off[-1])
    recs, _ = _integrate_chunk(c, ctxs, frames, 0, nf, nf > 1)
    # inside band 1's share of a frame: the last one in which the bands on either side of the cut have events
    shares = [np.bincount(_band_index(c, e), minlength=len(c["bands"])) for e in per]
    f = max(k for k in range(nf) if shares[k][0] > 0 and shares[k][1] >= 2)
    share = shares[f]
    assert 0 < f and int(want_off[f]) + int(share[0]) + int(share[1]) <= total
    inside = int(want_off[f]) + int(share[0]) + int(share[1]) // 2
    caps = [((total - 1) * rec, total - 1), (inside * rec, inside)]
    if form == "wire":
        caps.append(((total - 1) * rec - rec // 2, total - 2))
    root = ctxs[0]
    for cap_bytes, cap_events in caps:
        buf, moff = _Guarded(cap_bytes), _Offsets(nf + 1)
        _expand(root, form, recs, buf.out, 0, moff.out)
        with pytest.raises(A.AdderHipError) as ei:
            root.expand_status(stream=_stream())
        assert ei.value.code == A.E_OUT_CAPACITY
        buf.check(want, (name, form, cap_bytes), written=cap_events * rec)
        moff.check(want_off, (name, form, cap_bytes))
    buf, moff = _Guarded(total * rec), _Offsets(nf + 1)
    _expand(root, form, recs, buf.out, 0, moff.out)
    root.expand_status(stream=_stream())  # (the status word was cleared)
    buf.check(want, (name, form, "full"))
    moff.check(want_off, (name, form, "full"))


# ---- 5: the description block ring ----
@pytest.mark.parametrize("form", ["events", "wire"])
def test_description_blocks_are_reused_and_grow(form):
    """kBandDescSlots + 2 expansions of a one-band chunk with no host synchronisation between them (a slot is reused behind
    its event), then the 17 bands of one_row_bands_17 on the same root (the block is reallocated, larger, behind a
    stream synchronisation), then the one-band chunk again."""
    c = BC.case("one_row_bands_17", BC.DELTA_T)
    ctxs, frames = _bands_of(c, fresh=True)  # (a root whose block was sized by nothing yet)
    root = ctxs[0]
    per = BC.oracle_events(c["name"], c["time_mode"])
    rec = _rec(form, 1)
    f0 = 0
    for k, nf in enumerate(c["chunks"]):
        recs, _ = _integrate_chunk(c, ctxs, frames, f0, nf, nf > 1)
        own = [e[_band_index(c, e) == 0] for e in per[f0:f0 + nf]]  # band 0's events: the one-band chunk's stream
        want1, off1 = _bytes(own, form, 1), _offsets(own, 5 * k)
        singles = []
        for _ in range(BC.DESC_SLOTS + 2 if k == 0 else 1):
            buf, moff = _Guarded(5 * k * rec + len(want1)), _Offsets(nf + 1)
            _expand(root, form, recs[:1], buf.out, 5 * k, moff.out)
            singles.append((buf, moff))
        wantN, offN = _bytes(per[f0:f0 + nf], form, 1), _offsets(per[f0:f0 + nf])
        bufN, moffN = _Guarded(len(wantN)), _Offsets(nf + 1)
        _expand(root, form, recs, bufN.out, 0, moffN.out)
        if k == 1:  # ... and after the block has grown, the one-band chunk again
            buf, moff = _Guarded(5 * k * rec + len(want1)), _Offsets(nf + 1)
            _expand(root, form, recs[:1], buf.out, 5 * k, moff.out)
            singles.append((buf, moff))
        root.expand_status(stream=_stream())
        for i, (buf, moff) in enumerate(singles):
            buf.check(bytes([FILL]) * (5 * k * rec) + want1, ("one band", k, i), first=5 * k * rec)
            moff.check(off1, ("one band", k, i))
        bufN.check(wantN, ("17 bands", k))
        moffN.check(offN, ("17 bands", k))
        f0 += nf
    assert len(ctxs) == BC.MAX_BANDS + 1


# ---- 6: the wire image, several bands ----
def _align256(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("form", ["events", "wire"])
@pytest.mark.parametrize("name,time_mode,chunks", [("static_band", BC.DELTA_T, (4, 5, 4, 5)), ("rgb", BC.ABSOLUTE_T, None)])
def test_wire_image_of_several_bands(name, time_mode, chunks, form):
    """One image per band and chunk (adder_hip_records_to_wire -> adder_amd.records.records_from_wire); chunk k is expanded
    from the images alone AFTER the root has integrated chunk k + 1, with the frame table of the root's image: the root's
    own table is stale by then, and the D_EMPTY fillers' t comes from the copy.  static_band is cut into chunks of 4, 5, 4
    and 5 frames here, so that its middle band (still over frames 4 .. 13) has two chunks WITHOUT a record: their images
    end at the sixth section.  The sections are those include/adder_hip.h states; an image buffer one byte short is
    ADDER_E_BAD_PARAMS."""
    import torch
    A = _hip()
    from adder_amd import records as R
    c = BC.case(name, time_mode)
    chunks = list(c["chunks"] if chunks is None else chunks)
    ctxs, frames = _bands_of(c)
    root = ctxs[0]
    per = BC.oracle_events(name, time_mode)
    rec = _rec(form, c["Cn"])
    want, want_off = _bytes(per, form, c["Cn"]), _offsets(per)
    buf, moff = _Guarded(len(want)), _Offsets(len(per) + 1)
    pending, empty_images, f0 = None, 0, 0

    def expand_from(images, g0, nf):
        ftab = images[0][0].out.data_ptr() + R.wire_sections(nf, images[0][1].num_segments, images[0][1].record_bytes)[1]
        bands = [R.records_from_wire(img.out, nf, d.num_segments, d.record_bytes, d.row_begin, d.rows, d_frame_table=ftab)
                 for img, d in images]
        _expand(root, form, bands, buf.out, int(want_off[g0]), moff.out[g0:])
        root.expand_status(stream=_stream())

    for nf in chunks:
        recs, n_records = _integrate_chunk(c, ctxs, frames, f0, nf, nf > 1)
        images = []
        for r, hv in enumerate(ctxs):
            d = recs[r]
            sec = R.wire_sections(nf, d.num_segments, d.record_bytes)
            tab = _align256(nf * d.num_segments * 4)
            assert all(s % 256 == 0 for s in sec) and sec[0] == 0
            assert [sec[i + 1] - sec[i] for i in range(5)] == [_align256((nf + 1) * 8), _align256(nf * 8), tab, tab, tab]
            assert R.wire_bytes(nf, d.num_segments, d.record_bytes, 0) == sec[5]
            assert R.wire_bytes(nf, d.num_segments, d.record_bytes, n_records[r]) == \
                sec[5] + _align256(n_records[r] * (d.record_bytes & 0xff))
            if r == 1:
                with pytest.raises(A.AdderHipError) as ei:
                    _image_of(hv, d, n_records[r], short=1)
                assert ei.value.code == A.E_BAD_PARAMS
            img = _image_of(hv, d, n_records[r])
            empty_images += n_records[r] == 0
            images.append((img, d))
        if pending is not None:  # the chunk before, now that every band -- the root too -- has gone on
            expand_from(*pending)
        pending = (images, f0, nf)
        f0 += nf
    expand_from(*pending)
    torch.cuda.synchronize()
    for img, _ in pending[0]:  # (the copies stayed inside their images)
        host = img.big.cpu().numpy()
        assert (host[:GUARD] == FILL).all() and (host[GUARD + img.n:] == FILL).all()
    if name == "static_band":
        assert empty_images == 2
    moff.check(want_off, (name, form))
    buf.check(want, (name, form))


# ---- 7: refusals ----
def _copy(rec, **changes):
    out = type(rec).from_buffer_copy(rec)
    for k, v in changes.items():
        setattr(out, k, v)
    return out


@pytest.mark.parametrize("form", ["events", "wire"])
@pytest.mark.parametrize("kind", ["runs", "log"])
def test_refusals_leave_the_root_usable(monkeypatch, kind, form):
    """A root that never integrated, and every `band r: bad description`: ADDER_E_BAD_PARAMS, nothing written, and the
    next good call on the same root matches."""
    A = _hip()
    if kind == "log":
        monkeypatch.setenv("ADDER_HIP_NO_LR", "1")
    c = BC.case("rowlen_255", BC.ABSOLUTE_T)
    ctxs, frames = _bands_of(c)
    nf = c["chunks"][0]
    per = BC.oracle_events(c["name"], c["time_mode"])[:nf]
    rec = _rec(form, 1)
    want, want_off = _bytes(per, form, 1), _offsets(per)
    recs, _ = _integrate_chunk(c, ctxs, frames, 0, nf, kind == "runs")

    def refused(root, bands, tag, says):
        buf, moff = _Guarded(len(want)), _Offsets(nf + 1)
        with pytest.raises(A.AdderHipError) as ei:
            _expand(root, form, bands, buf.out, 0, moff.out)
        assert ei.value.code == A.E_BAD_PARAMS and says in str(ei.value), (tag, str(ei.value))
        root.expand_status(stream=_stream())
        buf.check(want, tag, written=0)
        moff.check(np.full(nf + 1, _Offsets.MARK), tag)

    def good(root, bands, tag):
        buf, moff = _Guarded(len(want)), _Offsets(nf + 1)
        _expand(root, form, bands, buf.out, 0, moff.out)
        root.expand_status(stream=_stream())
        buf.check(want, tag)
        moff.check(want_off, tag)

    # a root that never integrated: no frame table of its own
    fresh = _band_ctx(c, c["bands"][0])
    refused(fresh, recs, "fresh root", "root integrates the same frames first")
    own = fresh.integrate_records_device(frames[0][:nf], _live["boffs"][0], stream=_stream())  # (band 0's offsets again: the same values)
    fresh.finish()
    good(fresh, [own, recs[1]], "fresh root, after its own batch")
    fresh.close()
    root = ctxs[0]
    bad = {
        "num_frames": _copy(recs[1], num_frames=nf - 1),
        "record kind": _copy(recs[1], record_bytes=recs[1].record_bytes ^ RUNS),
        "num_segments": _copy(recs[1], num_segments=recs[1].num_segments + 1),
        "rows": _copy(recs[1], rows=0),
        "null table": _copy(recs[1], d_counts=None),
    }
    for tag, b in bad.items():
        refused(root, [recs[0], b], tag, "band 1: bad description")
        good(root, recs, ("after", tag))
