"""The compressed codec's source model on the device (include/adder_compressed_model.h, adder_amd.HipCompressedModel)
against the logic header run serially (tests/cpu_sim/compressed_model_main.cpp) and the host sink: device symbols ==
logic-header symbols word for word, reconstructed events == compressed_decode of the host encoder's stream.  Integer-
and bit-exact: no tolerances."""
import numpy as np
import pytest

import adder_amd as A
import compressed_model_cases as CM

pytestmark = pytest.mark.gpu

CASES = CM.gpu_cases()


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return CM.build_sim(tmp_path_factory.mktemp("compressed_model_sim"))


def _model(case, **kw):
    return A.HipCompressedModel(case["w"], case["h"], case["c"], ref_interval=case["ref"], adu_interval=case["adu"],
                                delta_t_max=case["dtm"], c_thresh_max=case["cmax"], tps=case["tps"], **kw)


def _collect(model, out):
    if not model.adus:
        return
    sym, ev = model.symbols_host(), model.events_host()
    so, eo = model.symbol_offsets.astype(np.int64), model.event_offsets.astype(np.int64)
    for a in range(model.adus):
        out["start_t"].append(int(model.start_t[a]))
        out["symbols"].append(sym[so[a]:so[a + 1]].copy())
        out["events"].append(ev[eo[a]:eo[a + 1]].copy())


def _run(case, events, cuts=()):
    """The stream through one model, cut into calls at `cuts` -> per ADU results, the ADUs each call closed, counters."""
    import torch
    model = _model(case)
    d = torch.from_numpy(np.ascontiguousarray(events).view(np.uint8).reshape(-1).copy()).cuda()
    out = {"start_t": [], "symbols": [], "events": []}
    closed = []
    edges = [0, *cuts, len(events)]
    for lo, hi in zip(edges[:-1], edges[1:]):
        closed.append(model.ingest(d[12 * lo:12 * hi]))
        _collect(model, out)
    closed.append(model.finish())
    _collect(model, out)
    assert model.open_adu()[0] == 0
    out["counters"] = model.counters()
    model.close()
    return out, closed


def _same(got, want):
    assert got["start_t"] == want["start_t"]
    assert len(got["symbols"]) == len(want["symbols"])
    for a, (g, w) in enumerate(zip(got["symbols"], want["symbols"])):
        assert len(g) == len(w) and np.array_equal(g, w), (a, len(g), len(w))
    for a, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert np.array_equal(g, w), a


_REF = {}


def _reference(case, sim, tmp_path):
    """Per case, computed once: the events, the logic header's results, the host sink's decoded events."""
    if case["name"] not in _REF:
        ev = case["events"]()
        want = CM.run_sim(sim, case, ev, tmp_path)
        dec = CM.decode(case, CM.host_stream(case, ev))
        _REF[case["name"]] = (ev, want, dec)
    return _REF[case["name"]]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_symbols_and_events_equal_the_host(case, sim, tmp_path):
    ev, want, dec = _reference(case, sim, tmp_path)
    got, closed = _run(case, ev)
    _same(got, want)
    assert np.array_equal(np.concatenate(got["events"]), dec)
    assert sum(closed) == len(want["symbols"]) and closed[-1] == 1
    c = got["counters"]
    assert (c["events_in"], c["events_dropped"], c["bitshift"]) == (want["events_in"], want["dropped"], want["bitshift"])
    if case["name"] == "g_dense_300":
        assert closed[0] >= 300          # one call that closes 300 ADUs
    if case["name"] == "g_long_lists":
        assert closed == [0, 1]          # one ADU, closed by close(): a pixel list of 65 and one of 4900
        key = ev["y"].astype(np.int64) * case["w"] + ev["x"]
        top = sorted(np.bincount(key))[-2:]                # (a few of the scattered events land on them too)
        assert 65 <= top[0] < 100 and 4900 <= top[1] < 4950


def test_symbol_path_gives_the_host_sinks_bytes():
    case = CASES[2]
    ev = case["events"]()
    out, recon = A.compress_events_device(ev, case["w"], case["h"], case["c"], tps=case["tps"], ref_interval=case["ref"],
                                          delta_t_max=case["dtm"], adu_interval=case["adu"], c_thresh_max=case["cmax"],
                                          threads=4, pieces=3)
    assert out == CM.host_stream(case, ev)
    rec = np.frombuffer(recon.cpu().numpy().tobytes(), A.EVENT_DTYPE)
    assert np.array_equal(rec, CM.decode(case, out))


def test_calls_cut_around_an_adu_cut_and_one_event_per_call(sim, tmp_path):
    case = next(c for c in CASES if c["name"] == "g_arms")
    ev, want, _ = _reference(case, sim, tmp_path)
    t, start, span = ev["t"].astype(np.int64), 0, case["ref"] * case["adu"]
    cut_at = []
    for i in range(len(ev)):
        if t[i] > start + span:
            cut_at.append(i)
            start += span
    assert len(cut_at) >= 3
    seen = set()
    for i in cut_at[:3]:
        for pos in range(max(1, i - 2), min(len(ev) - 1, i + 2) + 1):
            got, closed = _run(case, ev, cuts=(pos,))
            _same(got, want)
            seen.update(closed[:2])
    assert {0, 1} <= seen                  # calls that close no ADU, and one
    got, closed = _run(case, ev, cuts=tuple(range(1, len(ev))))   # one event per call
    _same(got, want)
    assert set(closed) == {0, 1}


def test_symbol_capacity_too_small_then_retry(sim, tmp_path):
    import torch
    case = next(c for c in CASES if c["name"] == "g160x144_adu1")
    ev, want, _ = _reference(case, sim, tmp_path)
    d = torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8).reshape(-1).copy()).cuda()
    half = len(ev) // 2
    model = _model(case, symbol_capacity=100)
    with pytest.raises(A.AdderHipError) as e:
        model.ingest(d[:12 * half])
    assert e.value.code == A.E_OUT_CAPACITY and e.value.needed > 100 and model.adus == 0
    assert model.open_adu() == (0, 0)      # nothing changed
    need = e.value.needed
    model.set_symbol_capacity(need - 1)
    with pytest.raises(A.AdderHipError) as e:
        model.ingest(d[:12 * half])
    assert e.value.code == A.E_OUT_CAPACITY and e.value.needed == need
    model.set_symbol_capacity(need)
    out = {"start_t": [], "symbols": [], "events": []}
    assert model.ingest(d[:12 * half]) > 0 and int(model.symbol_offsets[-1]) == need
    assert 0.0 < model.device_ms() < 1000.0   # the call's device share, by events
    _collect(model, out)
    model.set_symbol_capacity(None)
    model.ingest(d[12 * half:])
    _collect(model, out)
    model.finish()
    _collect(model, out)
    _same(out, want)
    model.close()


def test_refusals():
    import torch
    case = CASES[1]  # 17 x 33
    model = _model(case)
    bad = CM.events_of([(1, 1, 0xFF, 7, 5), (17, 1, 0xFF, 7, 6)])
    with pytest.raises(A.AdderHipError) as e:
        model.ingest(bad)
    assert e.value.code == A.E_BAD_PARAMS and model.open_adu() == (0, 0)
    with pytest.raises(A.AdderHipError):
        model.ingest(CM.events_of([(1, 33, 0xFF, 7, 5)]))
    with pytest.raises(A.AdderHipError):
        model.ingest(CM.events_of([(1, 1, 1, 7, 5)]))   # channel 1 of a one-channel plane
    assert model.ingest(torch.empty(0, dtype=torch.uint8, device="cuda")) == 0
    assert model.finish() == 0                            # no event: no ADU
    with pytest.raises(A.AdderHipError):
        model.ingest(CM.events_of([(1, 1, 0xFF, 7, 5)]))  # closed
    model.close()
    with pytest.raises(A.AdderHipError):
        A.HipCompressedModel(0, 10, 1, ref_interval=255, adu_interval=1)
    with pytest.raises(A.AdderHipError):
        A.HipCompressedModel(10, 10, 2, ref_interval=255, adu_interval=1)


def test_codec_loss_measured_on_the_device_equals_the_cpu_round_trip():
    """framer -> HipQuality on the model's reconstructed events (never leaving HBM) against the same metrics on the
    events the CPU round trip (encode, decode) gives: equal, frame for frame."""
    import torch
    from oracle import oracle as O
    W, H, T, dtm = 48, 40, 24, 7650
    clip = O.synth_clip(O.CONTENT_SCENE, W, H, 1, T)
    hv = A.HipVideo(W, H, 1, time_mode=A.TIME_ABSOLUTE_T, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=dtm)
    hv.set_crf_parameters(7, 7)
    hv.reset_c_thresh(2)
    d_clip = torch.from_numpy(clip.reshape(T, -1)).cuda()
    d_events = torch.empty(12 * 4 * W * H * T, dtype=torch.uint8, device="cuda")
    d_offsets = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv.integrate_device(d_clip, d_events, d_offsets, stream=torch.cuda.current_stream().cuda_stream)
    n = hv.finish()
    assert n > 1000
    case = dict(w=W, h=H, c=1, tps=7650, ref=255, dtm=dtm, adu=30, cmax=7, header=True)
    ev = np.frombuffer(d_events[:12 * n].cpu().numpy().tobytes(), A.EVENT_DTYPE)
    dec = CM.decode(case, CM.host_stream(case, ev, threads=4))

    kwf = dict(tps=7650, ref_interval=255, delta_t_max=dtm, output_fps=30.0, codec_version=3,
               time_mode=A.TIME_ABSOLUTE_T, source_camera=A.FRAMED_U8, ring_frames=256)
    q = A.HipQuality(W, H, 1, ssim=True)

    def metrics(feed):
        fr = A.HipFramer(W, H, 1, **kwf)
        d_out = torch.empty((T, W * H), dtype=torch.uint8, device="cuda")
        feed(fr)
        k = min(fr.frames_ready(), T)
        m = fr.pop_device(d_out, k) if k else 0
        while m < T and fr.flush_frame_buffer():   # Collapse holds frames back: the end-of-stream flush
            assert fr.pop_device(d_out[m:], 1) == 1
            m += 1
        fr.close()
        return m, q.compute_device(d_clip[:m], d_out[:m]), d_out[:m].cpu().numpy()

    model = _model(case)

    def feed_device(fr):
        for call in (lambda: model.ingest(d_events[:12 * n]), model.finish):
            if call():
                fr.ingest_device(model.events(), model.event_offsets)

    def feed_host(fr):
        fr.ingest(dec)

    m_dev, got, frames_dev = metrics(feed_device)
    m_cpu, want, frames_cpu = metrics(feed_host)
    model.close()
    assert m_dev == m_cpu and m_dev >= 4
    assert np.array_equal(frames_dev, frames_cpu)
    assert got == want
