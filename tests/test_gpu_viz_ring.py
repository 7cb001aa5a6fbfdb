"""The adder-viz player on the MI355X with pending rings that wrap (slot = frame % ring_frames): the streams, rings and
call plans of tests/viz_ring_cases.py (each stream at the smallest ring that holds it and at one more, cut into the
longest calls the player must accept), every frame and every P_j against the literal restatement, the popped form also
against the committed C checker.  Then the wrap's own edges: wire input, the default ring, finer cuts, a call that pops
exactly `ring` frames from a start that is not slot 0, refusals at a wrapped state that must change nothing, a limit
lowered at a wrapped state and a bad event inside a call that clears across the wrap.

What the plans reach is counted on the CPU (tests/test_viz_ring_cpu.py, CENSUS)."""
import functools

import numpy as np
import pytest

import viz_player_cases as K
import viz_ring_cases as RC
from viz_player_oracle import VizRestatement, ABSOLUTE_T, EVENT_DTYPE
from test_gpu_viz_player import play, same, to_device, NONE

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def planned(name, R):
    """-> cfg, events, cuts, restatement after finish, [(a, b, w0, n_pops)], frames before the drain"""
    cfg, ev = RC.stream(name)
    cuts = RC.plan(cfg, ev, R)
    r, calls, before = RC.replay(cfg, ev, cuts)
    return cfg, ev, cuts, r, calls, before


def play_ring(cfg, ev, cuts, ring, form, first_device, change=None):
    """The stream in the calls `cuts` delimits, device and host entry points in turn, then the finish drain.
    -> (frames [n, units], P_j), frames per call (the drain last), frames_written before every call and before the
    drain, the running frame after it"""
    from adder_amd import viz_player as V
    h = V.HipVizPlayer(form=form, ring_frames=ring, **cfg)
    frames, pops, counts, w0s = [], [], [], []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        device = (k % 2 == 0) == first_device
        if change is not None and change[0] == a:
            h.set_buffer_limit(change[1])
        w0s.append(h.frames_written)
        part = ev[a:b]
        got = h.ingest(to_device(part) if device and len(part) else part)  # a refusal raises: a planned call is accepted
        assert h.bad_index is None
        frames += list(got.cpu().numpy() if hasattr(got, "cpu") else got)
        pops += list(h.pop_index)
        counts.append(len(got))
    w0s.append(h.frames_written)
    got = h.finish(device=first_device)
    frames += list(got.cpu().numpy() if hasattr(got, "cpu") else got)
    pops += list(h.pop_index)
    counts.append(len(got))
    running = h.running_frame().reshape(-1).copy()
    h.close()
    n_units = cfg["width"] * cfg["height"] * cfg["channels"]
    return (np.array(frames, np.uint8).reshape(-1, n_units), [int(p) for p in pops]), counts, w0s, running


# ---- the full sweep ------------------------------------------------------------------------------------------------

CASES = RC.cases()


@pytest.mark.parametrize("name,R", CASES, ids=[f"{n}-ring{r}" for n, r in CASES])
def test_planned_calls_past_the_wrap(name, R):
    cfg, ev, cuts, r, calls, before = planned(name, R)
    assert before >= 3 * R  # the ring wrapped at least three times before the drain
    want_c = K.c_checker_frames(ev, cfg)
    for form, first_device in (("popped", True), ("running", False)):
        got, counts, w0s, running = play_ring(cfg, ev, cuts, R, form, first_device)
        assert w0s[:-1] == [c[2] for c in calls] and w0s[-1] == before
        assert counts[:-1] == [c[3] for c in calls] and counts[-1] == len(r.popped) - before
        same(got, r.popped, form)
        assert np.array_equal(running, r.running)
        if form == "popped":  # the committed C checker, directly
            assert got[1] == [p for p, _ in want_c]
            for k, (_, b) in enumerate(want_c):
                assert np.array_equal(got[0][k], b), k


def test_the_finish_drains_frames_from_wrapped_slots():
    """(of the sweep's cases) the drain starts at a frames_written that is no multiple of the ring and flushes frames"""
    hits = 0
    for name, R in CASES:
        _, _, _, r, _, before = planned(name, R)
        hits += int(before % R != 0 and r.flushes >= 2 and before >= R)
    assert hits >= 1


# ---- wire input, the default ring, finer cuts --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["7x5-abs-lim2", "4x3rgb-abs-lim2"])
def test_wire_input_past_the_wrap(name):
    R = RC.MIN_RING[name]
    cfg, ev, cuts, r, _, _ = planned(name, R)
    # play() checks `consumed` after every call
    same(play(cfg, ev, cuts, form="running", wire=True, device=True, ring_frames=R), r.popped, "running")
    same(play(cfg, ev, cuts, form="popped", wire=True, ring_frames=R), r.popped, "popped")


def test_the_default_ring_wraps():
    """ring_frames = 0: delta_t_max / tpf + 80 frames, what viz_play_file runs with"""
    from adder_amd import viz_player as V
    cfg, ev = RC.stream("7x5-dt-47fps-lim2")
    h = V.HipVizPlayer(ring_frames=0, **cfg)
    tpf = h.tpf
    h.close()
    assert tpf == VizRestatement(**cfg).tpf
    R = cfg["delta_t_max"] // tpf + 80
    cuts = RC.plan(cfg, ev, R)
    r, calls, before = RC.replay(cfg, ev, cuts)
    assert len(calls) >= 2 and before > R
    for form, first_device in (("popped", False), ("running", True)):
        got, counts, w0s, running = play_ring(cfg, ev, cuts, 0, form, first_device)
        assert w0s[-1] == before > R
        same(got, r.popped, form)
        assert np.array_equal(running, r.running)
    # one record more in the first call reaches frame `ring`: the default ring is this size and no larger
    h = V.HipVizPlayer(ring_frames=0, **cfg)
    import adder_amd as A
    with pytest.raises(A.AdderHipError) as ei:
        h.ingest(ev[:cuts[1] + 1])
    assert ei.value.code == A.E_OUT_CAPACITY and ei.value.needed == 0 and h.frames_written == 0
    h.close()


def test_finer_cuts_at_wrapped_states_give_the_same_frames():
    name, R = "7x5-abs-dvs-lim3", 7
    cfg, ev, cuts, r, calls, _ = planned(name, R)
    at = next(a for a, _, w0, _ in calls if w0 >= R and w0 % R != 0 and a >= len(ev) // 2)
    rng = np.random.default_rng(23)
    fine = sorted(cuts + K.random_splits(rng, len(ev), 9)[1:-1] + [at, at + 1])  # `at` twice: an empty call
    _, fcalls, _ = RC.replay(cfg, ev, fine)
    assert any(a == b and w0 >= R and w0 % R != 0 for a, b, w0, _ in fcalls)
    assert any(b - a == 1 and w0 >= R and w0 % R != 0 for a, b, w0, _ in fcalls)
    got, _, w0s, running = play_ring(cfg, ev, fine, R, "running", True)
    assert w0s[:-1] == [c[2] for c in fcalls]
    same(got, r.popped, "running")
    got, _, _, _ = play_ring(cfg, ev, fine, R, "popped", False)
    same(got, r.popped, "popped")


# ---- a full ring in one call ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ring", [4, 5])
def test_a_call_that_pops_the_whole_ring_from_carried_slots(ring):
    """2x1, no limit: both units at frame 3, unit A fills the `ring` pending frames 3 .. ring + 2 (the last one on the
    ring's last slot for this w0; all but the first ring - 3 in wrapped slots), then unit B completes all of them in
    a call of its own: `ring` pops, the clear in two pieces, A's bytes from the carried ring.  Then frame after frame:
    the cleared slots hold no stale Some and no stale count."""
    cfg = K.base_cfg(2, 1, 1, buffer_limit=None)
    A_, B_ = 0, 1
    steps = [(A_, 3, 5), (B_, 3, 4), (A_, ring, 7), (B_, ring, 6)]  # unit, frames it advances, D
    cuts = [0, 2, 3, 4]
    d = 1
    for calls_of in ([(A_, B_)], [(A_, B_)], [(A_,), (B_,)], [(B_,), (A_,)], [(A_, B_)], [(A_, B_)], [(A_, B_)]):
        for call in calls_of:
            for u in call:
                steps.append((u, 1, d % 8))
                d += 3
            cuts.append(len(steps))
    ev = np.zeros(len(steps), EVENT_DTYPE)
    for i, (u, k, dd) in enumerate(steps):
        ev[i] = (u, 0, NONE, dd, 0, 255 * k)
    r, calls, before = RC.replay(cfg, ev, cuts)
    assert [c[3] for c in calls[:3]] == [3, 0, ring] and calls[2][2] == 3 and before == ring + 3 + 7
    row, frm, to, last, unit = RC.chain(cfg, ev)
    assert to[2] == 3 + ring - 1  # the ring's last slot
    for k in range(3, 3 + ring):  # A's and B's bytes differ and are not the None byte
        assert r.popped[k][1][A_] != r.popped[k][1][B_] and r.popped[k][1].all() and r.popped[k][2].all()
    for form, first_device in (("popped", True), ("running", False)):
        got, counts, w0s, running = play_ring(cfg, ev, cuts, ring, form, first_device)
        assert counts[:3] == [3, 0, ring] and w0s[:4] == [0, 3, 3, 3 + ring]
        assert counts[:-1] == [c[3] for c in calls]
        same(got, r.popped, form)
        assert np.array_equal(running, r.running)


# ---- refusals at a wrapped state -----------------------------------------------------------------------------------------

def _frames(got):
    return list(got.cpu().numpy() if hasattr(got, "cpu") else got)


def test_refusals_at_a_wrapped_state_change_nothing():
    """a merged call whose fills pass the ring (the plan had to cut there), and a call that clears across the wrap with
    room for one frame less than it pops: both refused, and every later frame as if they had not been tried"""
    import adder_amd as A
    from adder_amd import viz_player as V
    name, R = "7x5-abs-lim2", 6
    cfg, ev, cuts, r, calls, _ = planned(name, R)
    _, frm, to, _, _ = RC.chain(cfg, ev)
    deep = next(k for k, (a, b, w0, _) in enumerate(calls[:-1])
                if w0 >= R and w0 % R != 0 and a >= len(ev) // 3 and to[b] > frm[b] and to[b] >= w0 + R)
    short = next(k for k, (a, b, w0, n) in enumerate(calls) if k > deep + 1 and w0 % R != 0 and w0 % R + n > R)
    for form, device in (("popped", True), ("running", False)):
        h = V.HipVizPlayer(form=form, ring_frames=R, **cfg)
        frames, pops = [], []
        for k, (a, b, w0, n) in enumerate(calls):
            feed = (lambda part: to_device(part)) if device else (lambda part: part)
            assert h.frames_written == w0
            if k == deep:
                with pytest.raises(A.AdderHipError) as ei:
                    h.ingest(feed(ev[a:calls[k + 1][1]]))
                assert ei.value.code == A.E_OUT_CAPACITY and ei.value.needed == 0 and h.frames_written == w0
            if k == short:
                with pytest.raises(A.AdderHipError) as ei:
                    h.ingest(feed(ev[a:b]), max_frames=n - 1)
                assert ei.value.code == A.E_OUT_CAPACITY and ei.value.needed == n and h.frames_written == w0
                got = h.ingest(feed(ev[a:b]), max_frames=n)  # the same call with room
            else:
                got = h.ingest(feed(ev[a:b]))
            assert len(got) == n
            frames += _frames(got)
            pops += list(h.pop_index)
        frames += _frames(h.finish(device=device))
        pops += list(h.pop_index)
        same((np.array(frames, np.uint8).reshape(len(frames), -1), [int(p) for p in pops]), r.popped, form)
        assert np.array_equal(h.running_frame().reshape(-1), r.running)
        h.close()


# ---- a lowered limit and a bad event at a wrapped state ------------------------------------------------------------------

def test_lowering_the_limit_at_a_wrapped_state():
    """7x5 AbsoluteT, limit 60 -> 1 in front of a planned call whose frames_written is no multiple of the ring: the
    loop in front of the read loop pops from carried counts and trackers in wrapped slots"""
    w, h_, c, n, _, _, cam, fps, _ = RC.STREAMS["7x5-abs-lim2"]
    cfg = K.base_cfg(w, h_, c, time_mode=ABSOLUTE_T, buffer_limit=60, source_camera=cam, output_fps=fps)
    ev = RC.stream("7x5-abs-lim2")[1]
    R = RC.min_ring(cfg, ev)  # the ring the limit-60 stream needs
    change = RC.limit_change(cfg, ev, R, RC.plan(cfg, ev, R), limit=1)
    assert change is not None
    cuts = RC.plan(cfg, ev, R, change)  # planned again with the restatement that applies the change
    r, calls, _ = RC.replay(cfg, ev, cuts, change)
    at = [k for k, c_ in enumerate(calls) if c_[0] == change[0]][0]
    assert calls[at][2] >= R and calls[at][2] % R != 0
    opening = [p for p in r.popped if p[0] == change[0] - 1]
    assert len(opening) >= 2 and r.popped[calls[at][2]][0] == change[0] - 1  # the call's first pops are the opening's
    for form, first_device in (("running", True), ("popped", False)):
        got, counts, w0s, running = play_ring(cfg, ev, cuts, R, form, first_device, change=change)
        assert counts[:-1] == [c_[3] for c_ in calls] and w0s[:-1] == [c_[2] for c_ in calls]
        same(got, r.popped, form)
        assert np.array_equal(running, r.running)


def test_a_bad_event_in_a_call_that_clears_across_the_wrap():
    from adder_amd import viz_player as V
    name, R = "7x5-abs-lim2", 6
    cfg, ev, cuts, r, calls, _ = planned(name, R)

    W, _ = RC.ahead(cfg, ev)  # frames_written in front of every event
    # a call whose first half alone already pops across the end of the ring; the bad event sits in its middle
    k = next(k for k, (a, b, w0, n) in enumerate(calls)
             if w0 >= R and w0 % R != 0 and b - a >= 4 and w0 % R + (W[(a + b) // 2] - w0) > R)
    a, b, w0, n = calls[k]
    bad_at = (a + b) // 2
    n_first = int(W[bad_at] - w0)
    bad = ev[a:b].copy()
    bad["x"][bad_at - a] = cfg["width"]  # outside the plane
    h = V.HipVizPlayer(form="running", ring_frames=R, **cfg)
    frames, pops = [], []
    for j, (a_, b_, w0_, n_) in enumerate(calls):
        if j == k:
            got = h.ingest(to_device(bad))
            assert h.bad_index == bad_at - a and len(got) == n_first and h.frames_written == w0 + n_first
            frames += _frames(got)
            pops += list(h.pop_index)
            got = h.ingest(ev[bad_at:b])  # the stream goes on from that event as if the call had ended before it
            assert h.bad_index is None and len(got) == n - n_first
        else:
            got = h.ingest(ev[a_:b_] if j % 2 else to_device(ev[a_:b_]))
            assert h.bad_index is None and len(got) == n_
        frames += _frames(got)
        pops += list(h.pop_index)
    frames += _frames(h.finish())
    pops += list(h.pop_index)
    same((np.array(frames, np.uint8).reshape(len(frames), -1), [int(p) for p in pops]), r.popped, "running")
    assert np.array_equal(h.running_frame().reshape(-1), r.running)
    h.close()
