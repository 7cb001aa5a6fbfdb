"""The batch modes enqueue_frames is asked for (csrc/adder_hip_ctx.hpp BatchRequest) that no other GPU test reaches:
timed launches, the per-frame ring on three slots (the frame-only split) and on four (the whole pipeline on one stream)
in both output formats and in feature mode, and a records-only batch in both record kinds followed by an ordinary batch
on the same context.  Every mode's events equal, bit for bit, those of adder_hip_integrate_batch on a fresh context.
The plane is 66 x 50 x 1: 3300 units, no whole number of segments."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import clips

W, H = 66, 50
RECORDS_RUNS = 0x100  # ADDER_RECORDS_RUNS (include/adder_hip.h)

# regime -> (HipVideo arguments, (c_thresh baseline, c_thresh_max, c_increase_velocity), clip kind)
REGIMES = {
    # the lossless corner: the packed lean-runs kernel
    "lean": (dict(time_mode=O.DELTA_T, multi_mode=O.COLLAPSE, ref_time=255, delta_t_max=255), (0, 0, 10), "runs"),
    # the reference's defaults: per-event records
    "default": (dict(time_mode=O.DELTA_T, multi_mode=O.COLLAPSE, ref_time=255, delta_t_max=7650), (2, 7, 7), "runs"),
    # feature-driven rate control (the feature loop; per-unit thresholds)
    "features": (dict(time_mode=O.ABSOLUTE_T, multi_mode=O.COLLAPSE, ref_time=255, delta_t_max=255, max_depth=30), (2, 7, 7),
                 "corners"),
}
FRAMES = 16
_reference = {}


def _hip():
    import adder_amd
    return adder_amd


def _video(regime):
    A = _hip()
    kw, (base, cmax, vel), _ = REGIMES[regime]
    hv = A.HipVideo(W, H, 1, **kw)
    hv.set_crf_parameters(cmax, vel)
    hv.reset_c_thresh(base)
    if regime == "features":
        hv.update_detect_features(True, True)
        hv.set_feature_parameters(2, 3)
    return hv


def _ref(regime):
    """(clip, events per frame, new features per frame) of the blocking path: adder_hip_integrate_batch, frame by frame,
    on a fresh context.  Computed once per regime."""
    if regime not in _reference:
        clip = clips.make_clip(REGIMES[regime][2], FRAMES, H, W, 1, seed=41)
        hv = _video(regime)
        events, feats = [], []
        for f in clip:
            ev, _ = hv.integrate_batch(f[None])
            events.append(ev)
            feats.append(hv.last_new_features())
        hv.close()
        assert sum(len(e) for e in events) > 1000
        _reference[regime] = (clip, events, feats)
    return _reference[regime]


def _device_batch(hv, frames):
    """adder_hip_integrate_device + finish -> the batch's events"""
    import torch
    T = len(frames)
    d_frames = torch.from_numpy(np.ascontiguousarray(frames).reshape(T, -1)).cuda()
    d_events = torch.empty((hv.max_events_per_frame * T, 3), dtype=torch.int32, device="cuda")
    d_offsets = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv.integrate_device(d_frames, d_events, d_offsets, stream=torch.cuda.current_stream().cuda_stream)
    n = hv.finish()
    return np.frombuffer(d_events[:n].cpu().numpy().tobytes(), dtype=_hip().EVENT_DTYPE)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("regime", ["lean", "default"])
def test_timed_launches_produce_the_untimed_events(regime, mode):
    """adder_hip_set_launch_timing 1 (an event pair around every frame-kernel launch) and 2 (around a chunk's run of them):
    the eager loop, the same events."""
    clip, want, _ = _ref(regime)
    hv = _video(regime)
    hv.set_launch_timing(mode)
    got = []
    for f0, f1 in ((0, 9), (9, 10), (10, FRAMES)):  # nine frames, one frame (the scan writes its offsets), the rest
        ev, offs = hv.integrate_batch(clip[f0:f1])
        assert [int(offs[k + 1] - offs[k]) for k in range(f1 - f0)] == [len(w) for w in want[f0:f1]]
        assert hv.last_launch_avg_us() > 0.0 and hv.last_post_chunks() == 1
        got.append(ev)
    assert np.array_equal(np.concatenate(got), np.concatenate(want))
    hv.set_launch_timing(0)  # and untimed again on the same context: back on the captured path, the stream goes on
    extra = clips.make_clip("runs", 3, H, W, 1, seed=42)
    a, _ = hv.integrate_batch(extra)
    assert hv.last_launch_avg_us() == 0.0
    hv.close()
    fresh = _video(regime)
    fresh.integrate_batch(clip)
    b, _ = fresh.integrate_batch(extra)
    fresh.close()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("wire", [False, True], ids=["events", "wire"])
@pytest.mark.parametrize("slots,frames", [(3, 7), (4, 9)])
@pytest.mark.parametrize("regime", ["lean", "default", "features"])
def test_frame_ring_then_blocking_call_then_device_batch(regime, slots, frames, wire):
    """The per-frame ring with its slots' own batch descriptions: 7 frames on 3 slots (only the frame kernel on the
    context's stream) and 9 on 4 (the whole pipeline on it), AdderEvents and wire records, the slot's own feature
    counters; then adder_hip_integrate into page-locked memory and a device batch with the context's own description."""
    clip, want, want_feats = _ref(regime)
    hv = _video(regime)
    hv.frames_configure(slots, 0)
    hv.frames_set_format(wire)
    pinned = [hv.pinned_frame() for _ in range(slots)]
    got, feats = [], []

    def collect():
        got.append(hv.frame_collect_wire() if wire else hv.frame_collect())
        feats.append(hv.last_new_features())

    for k in range(frames):
        if hv.frames_in_flight() == slots:
            collect()
        pinned[k % slots][...] = clip[k].reshape(H, W)
        hv.frame_submit(pinned[k % slots])
    assert hv.frames_in_flight() == slots
    while hv.frames_in_flight():
        collect()
    assert len(got) == frames
    for k in range(frames):
        if wire:
            data, n = got[k]
            assert n == len(want[k]) and data.tobytes() == O.raw_events(want[k], 1), k
        else:
            assert np.array_equal(got[k], want[k]), k
    if regime == "features":
        assert feats == want_feats[:frames] and sum(feats) > 0
    # the blocking per-frame call (its event buffer is page-locked: the events go straight into it) ...
    assert np.array_equal(hv.integrate_matrix(clip[frames]), want[frames])
    if regime == "features":
        assert hv.last_new_features() == want_feats[frames]
    # ... and a device batch on the same context
    assert np.array_equal(_device_batch(hv, clip[frames + 1:frames + 4]), np.concatenate(want[frames + 1:frames + 4]))
    hv.close()


@pytest.mark.parametrize("kind", ["runs", "log"])
def test_records_batch_then_an_ordinary_batch(monkeypatch, kind):
    """adder_hip_integrate_records_device in both record kinds (lean runs; lean log with the lean-runs kernel switched
    off), expanded on the same context; then an ordinary batch: it expands its events and keeps its undo copy -- a buffer
    one event short is rolled back and the retry matches."""
    import torch
    A = _hip()
    if kind == "log":
        monkeypatch.setenv("ADDER_HIP_NO_LR", "1")
    clip, want, _ = _ref("lean")
    hv = _video("lean")
    st = torch.cuda.current_stream().cuda_stream
    T = 11
    d_frames = torch.from_numpy(np.ascontiguousarray(clip[:T]).reshape(T, -1)).cuda()
    d_offsets = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    rec = hv.integrate_records_device(d_frames, d_offsets, stream=st)
    n = hv.finish()
    assert bool(rec.record_bytes & RECORDS_RUNS) == (kind == "runs")
    assert n == sum(len(w) for w in want[:T]) and 0 < hv.last_batch_records() <= n
    d_merged = torch.empty((n + 16, 3), dtype=torch.int32, device="cuda")
    d_moff = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv.expand_records_device([rec], d_merged, 0, d_moff, stream=st)
    hv.expand_status(stream=st)
    assert d_merged[:n].cpu().numpy().tobytes() == np.concatenate(want[:T]).tobytes()
    assert d_moff.cpu().tolist() == np.cumsum([0] + [len(w) for w in want[:T]]).tolist()
    # no mode is left behind on the context
    rest = np.concatenate(want[T:])
    with pytest.raises(A.AdderHipError) as ei:
        hv.integrate_batch(clip[T:], out_cap=len(rest) - 1)
    assert ei.value.code == A.E_OUT_CAPACITY and hv.last_required == len(rest)
    got, _ = hv.integrate_batch(clip[T:], out_cap=len(rest))
    assert np.array_equal(got, rest)
    hv.close()
