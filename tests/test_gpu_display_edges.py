"""The display frame (adder_hip_display_frame[_device], csrc/adder_display.hip) past one tile, after batches, after the
per-frame ring, after a refused batch and after a reset -- byte for byte against the CPU oracle (oracle.Video's plane,
feature set and new features, the crosses drawn by live_view_oracle.draw_crosses).  The inputs are tests/display_cases.py;
tests/test_display_cases_cpu.py shows on the oracle alone that they reach what they are built for."""
import numpy as np
import pytest

import display_cases as D
import live_view_oracle as R

pytestmark = pytest.mark.gpu

SHOWS = [R.SHOW_OFF, R.SHOW_INSTANT, R.SHOW_HOLD]
SHOW_IDS = ["off", "instant", "hold"]
GUARD = 0xA5
OFFSETS = (0, 1, 4, 15)   # of the destination, in bytes: aligned, odd, a dword, the last byte of a line


def _hip():
    import adder_amd
    return adder_amd


def _same_display(hv, want, what):
    got = hv.display_frame()
    assert np.array_equal(got, want), (what, D.first_difference(got, want))


# ---- 1. across tiles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("show", SHOWS, ids=SHOW_IDS)
@pytest.mark.parametrize("W,H,Cn", D.PLANES, ids=D.PLANE_IDS)
def test_display_across_tiles(W, H, Cn, show):
    """Two and three tiles per row, a last tile of 5 bytes and one of 4 pixels, crosses on every tile boundary in x and on
    the row tiles' edges; into the context's staging buffer and into caller memory at four alignments, guard bytes around."""
    import torch
    A = _hip()
    assert D.tiles_per_row(W, Cn) >= 2
    clip, steps = D.edge_clip(W, H, Cn), D.edge_trace(W, H, Cn)
    hv = D.hip_video(A, W, H, Cn, show)
    n = W * H * Cn
    stream = torch.cuda.current_stream().cuda_stream
    for k, want in enumerate(steps):
        assert np.array_equal(hv.integrate_matrix(clip[k]), want.events), k
        assert np.array_equal(hv.feature_set(), want.feature_set), k
        _same_display(hv, want.display[show], k)
        for off in OFFSETS:
            buf = torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
            hv.display_frame_device(buf[off:off + n], stream=stream)
            got = buf.cpu().numpy()
            assert (got[:off] == GUARD).all() and (got[off + n:] == GUARD).all(), (k, off)
            got = got[off:off + n].reshape(H, W, Cn)
            assert np.array_equal(got, want.display[show]), (k, off, D.first_difference(got, want.display[show]))
    hv.close()


# ---- 2. after batches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("show", SHOWS[1:], ids=SHOW_IDS[1:])
@pytest.mark.parametrize("W,H,Cn", D.SMALL_PLANES)
def test_display_after_batches(W, H, Cn, show):
    """Frame f of a batch stamps frames_done + 1 + f; the display compares with frames_done after the batch: batches of 5,
    1 and 3 frames, each ending on a frame that finds new features and holds older ones."""
    A = _hip()
    clip = D.batch_clip(W, H, Cn)
    steps = D.trace(W, H, Cn, clip)
    hv = D.hip_video(A, W, H, Cn, show)
    lo = 0
    for nb in D.BATCHES:
        got, offs = hv.integrate_batch(clip[lo:lo + nb], out_cap=hv.max_events_per_frame * nb)
        assert np.array_equal(got, np.concatenate([s.events for s in steps[lo:lo + nb]])), lo
        last = steps[lo + nb - 1]
        assert np.array_equal(hv.feature_set(), last.feature_set), lo
        _same_display(hv, last.display[show], (lo, nb))
        lo += nb
    hv.close()


# ---- 3. after the per-frame ring ----------------------------------------------------------------------------------------
def test_display_after_the_frame_ring():
    """Three frames in flight, every frame queued with its own stamp; Instant shows what the last frame found new."""
    A = _hip()
    W, H, Cn = D.RING_PLANE
    clip = D.ring_clip()
    events, last, _ = D.ring_trace()
    _, hv = D.ring_pair(A)
    hv.set_show_features(R.SHOW_INSTANT)
    pinned = [hv.pinned_frame() for _ in range(D.RING_IN_FLIGHT)]
    got = []
    for k, f in enumerate(clip):
        if hv.frames_in_flight() == D.RING_IN_FLIGHT:
            got.append(hv.frame_collect())
        pinned[k % D.RING_IN_FLIGHT][...] = f.reshape(H, W * Cn)
        hv.frame_submit(pinned[k % D.RING_IN_FLIGHT])
    assert hv.frames_in_flight() == D.RING_IN_FLIGHT
    while hv.frames_in_flight():
        got.append(hv.frame_collect())
    assert len(got) == len(events)
    for k, (a, b) in enumerate(zip(events, got)):
        assert np.array_equal(a, b), k
    assert np.array_equal(hv.feature_set(), last.feature_set)
    _same_display(hv, last.display[R.SHOW_INSTANT], "ring")
    hv.close()


# ---- 4. after a refused batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("show", SHOWS[1:], ids=SHOW_IDS[1:])
def test_display_after_a_refused_batch(show):
    """A batch refused for its event buffer has run its feature passes; the rollback leaves nothing of them behind: clip B,
    stepped behind the refusal, gives the events, the feature set and the display of a video that never saw clip A.

    Run once against a library without the undo copy of the feature stamps (AdderHipCtx::Snapshot::fstamp), the Instant
    case failed behind B's frame 0: 18 bytes differed, the first at byte 430 (x 10, y 6) -- the crosses of (10, 8) and
    (30, 8), which clip A's frame 0 had made new.  The Hold case passed there: the feature set was always rolled back."""
    A = _hip()
    W, H, Cn = D.RB_PLANE
    prefix, a, b = D.rollback_clips()
    ta, tb = D.rollback_traces()
    F = len(prefix)
    hv = D.hip_video(A, W, H, Cn, show)
    for k in range(F):
        assert np.array_equal(hv.integrate_matrix(prefix[k]), tb[k].events), k
    need = sum(len(s.events) for s in ta[F:])
    with pytest.raises(A.AdderHipError) as ei:
        hv.integrate_batch(a, out_cap=need - 1)
    assert ei.value.code == A.E_OUT_CAPACITY
    assert np.array_equal(hv.feature_set(), tb[F - 1].feature_set)
    _same_display(hv, tb[F - 1].display[show], "behind the refusal")
    for k in range(len(b)):
        want = tb[F + k]
        assert np.array_equal(hv.integrate_matrix(b[k]), want.events), k
        assert np.array_equal(hv.feature_set(), want.feature_set), k
        _same_display(hv, want.display[show], k)
    hv.close()


# ---- 5. after a reset ---------------------------------------------------------------------------------------------------
def test_display_after_reset():
    """adder_hip_reset clears the stamps with the feature set: clip B behind clip A and a reset equals clip B on a freshly
    created context and on the oracle, frame by frame."""
    A = _hip()
    W, H, Cn = D.RB_PLANE
    _, a, b = D.rollback_clips()
    want = D.trace(W, H, Cn, b)
    assert sum(len(s.new) for s in want) == len(D.RB_ON_B)
    hv = D.hip_video(A, W, H, Cn, R.SHOW_INSTANT)
    for f in a:
        hv.integrate_matrix(f)
    assert hv.feature_set().any()
    hv.reset()
    D.apply_parameters(hv, R.SHOW_INSTANT)
    fresh = D.hip_video(A, W, H, Cn, R.SHOW_INSTANT)
    for k in range(len(b)):
        ev, ev_fresh = hv.integrate_matrix(b[k]), fresh.integrate_matrix(b[k])
        assert np.array_equal(ev, want[k].events) and np.array_equal(ev_fresh, want[k].events), k
        assert np.array_equal(hv.feature_set(), want[k].feature_set), k
        assert np.array_equal(fresh.display_frame(), want[k].display[R.SHOW_INSTANT]), k
        _same_display(hv, want[k].display[R.SHOW_INSTANT], k)
    hv.close()
    fresh.close()
