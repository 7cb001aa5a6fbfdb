"""The adder-viz player's pending ring where it wraps, on the CPU: (1) the streams, rings and call plans of
tests/viz_ring_cases.py and a census of what they reach, by the literal restatement alone; (2) the product's pop
schedule (viz_schedule, built by g++ in tests/cpu_sim/viz_carry_sim.cpp) driven call after call with those small rings,
so that its carried inputs -- cnt_carry, done_carry, m0, opening and w0 > 0 -- are not trivially zero, against the
restatement in P_j, in the flushed count and in the Some masks.

CENSUS below is what the committed streams give (test_census prints it with -s and compares).  Per (stream, ring): at
least 3 wraps of the ring before the drain, at least 2 calls whose pops straddle the end of the ring from a start that
is not slot 0, at least 2 calls with a fill on the ring's last slot, and for the limited streams a None in at least a
third of the frames popped before the drain.
"""
import numpy as np
import pytest

import viz_ring_cases as RC
import viz_carry_sim_py as SIM
from viz_player_oracle import some_masks_from_schedule

# (stream, ring): calls, frames before the drain, wraps, across-wrap clears, last-slot calls, most pops in one call,
# frames with a None
CENSUS = {
    ('7x5-abs-lim2', 6): (33, 112, 18, 12, 32, 5, 88),
    ('7x5-abs-lim2', 7): (27, 112, 16, 13, 26, 6, 88),
    ('7x5-abs-lim1', 5): (35, 113, 22, 19, 34, 5, 107),
    ('7x5-abs-lim1', 6): (28, 113, 18, 15, 27, 5, 107),
    ('7x5-abs-dvs-lim3', 7): (32, 111, 15, 10, 31, 6, 85),
    ('7x5-abs-dvs-lim3', 8): (27, 111, 13, 13, 26, 6, 85),
    ('4x3rgb-abs-lim2', 4): (40, 87, 21, 5, 40, 3, 60),
    ('4x3rgb-abs-lim2', 5): (37, 87, 17, 10, 36, 4, 60),
    ('7x5-dt-lim2', 26): (8, 145, 5, 5, 6, 24, 140),
    ('7x5-dt-lim2', 27): (8, 145, 5, 5, 6, 25, 140),
    ('7x5-dt-47fps-lim2', 37): (8, 200, 5, 5, 5, 35, 199),
    ('7x5-dt-47fps-lim2', 38): (8, 200, 5, 5, 6, 35, 199),
    ('3x70-abs-lim2', 10): (6, 38, 3, 2, 6, 8, 33),
    ('3x70-abs-lim2', 11): (6, 38, 3, 3, 5, 8, 33),
    ('257x3-abs-lim2', 4): (14, 25, 6, 6, 13, 2, 24),
    ('257x3-abs-lim2', 5): (12, 25, 5, 2, 12, 3, 24),
    ('5x4-abs-nolimit', 2): (55, 100, 50, 21, 54, 2, 0),
    ('5x4-abs-nolimit', 3): (37, 100, 33, 20, 37, 3, 0),
    ('5x4-dt-nolimit', 17): (27, 120, 7, 4, 22, 12, 0),
    ('5x4-dt-nolimit', 18): (22, 120, 6, 6, 17, 12, 0),
}


@pytest.fixture(scope="module")
def planned():
    """every (stream, ring) once: name, ring, cfg, events, cuts"""
    out = []
    for name, R in RC.cases():
        cfg, ev = RC.stream(name)
        out.append((name, R, cfg, ev, RC.plan(cfg, ev, R)))
    return out


def test_the_rings_are_the_smallest_that_hold_the_streams():
    for name in RC.STREAMS:
        cfg, ev = RC.stream(name)
        W, to = RC.ahead(cfg, ev)
        m = RC.min_ring(cfg, ev)
        assert int((to - W[:-1]).max()) == m - 1 and m == RC.MIN_RING[name]
        assert (name, m) in RC.cases() and (name, m + 1) in RC.cases()
        with pytest.raises(AssertionError):
            RC.plan(cfg, ev, m - 1)


def test_census(planned):
    got = {}
    for name, R, cfg, ev, cuts in planned:
        c = RC.census(cfg, ev, R, cuts)
        got[(name, R)] = (c["calls"], c["before_drain"], c["wraps"], c["across"], c["last_slot"], c["max_pops"],
                          c["with_none"])
        print(f"    {(name, R)!r}: {got[(name, R)]!r},")
        assert c["wraps"] >= 3 and c["across"] >= 2 and c["last_slot"] >= 2, (name, R, c)
        if cfg["buffer_limit"] is not None:
            assert 3 * c["with_none"] >= c["before_drain"] > 0, (name, R, c)
    assert got == CENSUS


def _run_sim(name, R, cfg, ev, cuts, change=None):
    """the plan through the carried schedule: -> the restatement, P_j, flushed marks, whether an opening loop popped"""
    r, calls, _ = RC.replay(cfg, ev, cuts, change)
    row, frm, to, last, unit = RC.chain(cfg, ev)
    sim = SIM.CarrySim(cfg["height"], cfg["width"] * cfg["channels"], R, cfg["buffer_limit"])
    pops, flushed, opened = [], [], False
    for a, b, w0, n_pops in calls:
        assert sim.w == w0, (name, R, a)
        if change is not None and change[0] == a:
            sim.set_buffer_limit(change[1])
        got = sim.call(row[a:b], frm[a:b], to[a:b], last[a:b])
        assert got != SIM.REFUSED, (name, R, a, b)  # a planned call is accepted
        assert len(got[0]) == n_pops, (name, R, a, b)
        opened |= any(p == a - 1 for p in got[0]) and change is not None and change[0] == a
        pops += got[0]
        flushed += list(got[1])
    got = sim.call(row[:0], frm[:0], to[:0], last[:0], finish=True)
    pops += got[0]
    flushed += list(got[1])
    assert pops == [p[0] for p in r.popped], (name, R)
    assert int(np.sum(flushed)) == r.flushes, (name, R)
    some = some_masks_from_schedule(pops, frm, to, unit, cfg["width"] * cfg["height"] * cfg["channels"])
    for k, (_, _, wsome, _) in enumerate(r.popped):
        if flushed[k]:
            assert wsome.all(), (name, R, k)
        else:
            assert np.array_equal(some[k], wsome), (name, R, k)
    return r, opened


def test_the_carried_schedule_matches_the_restatement(planned):
    for name, R, cfg, ev, cuts in planned:
        _run_sim(name, R, cfg, ev, cuts)


def test_the_carried_schedule_with_a_limit_lowered_at_a_wrapped_state(planned):
    """set_buffer_limit(1) between two planned calls where frames_written % ring != 0: the next call opens with the
    loop in front of the read loop, on carried counts and trackers"""
    ran = opened_in = 0
    for name, R, cfg, ev, cuts in planned:
        if cfg["buffer_limit"] == 1:
            continue
        change = RC.limit_change(cfg, ev, R, cuts)
        if change is None:
            continue
        cuts2 = RC.plan(cfg, ev, R, change)
        assert change[0] in cuts2
        _, opened = _run_sim(name, R, cfg, ev, cuts2, change)
        ran += 1
        opened_in += int(opened)
    assert ran >= 8 and opened_in >= 4


def test_the_sim_refuses_a_fill_past_the_ring_and_changes_nothing(planned):
    name, R, cfg, ev, cuts = planned[0]
    row, frm, to, last, _ = RC.chain(cfg, ev)
    sim = SIM.CarrySim(cfg["height"], cfg["width"] * cfg["channels"], R, cfg["buffer_limit"])
    sim.call(row[:cuts[1]], frm[:cuts[1]], to[:cuts[1]], last[:cuts[1]])
    before = (sim.w, sim.m, sim.n_events, sim.cnt.copy(), sim.done.copy())
    a, b = cuts[1], cuts[3]  # two planned calls as one: the plan had to cut between them
    assert sim.call(row[a:b], frm[a:b], to[a:b], last[a:b]) == SIM.REFUSED
    assert (sim.w, sim.m, sim.n_events) == before[:3]
    assert np.array_equal(sim.cnt, before[3]) and np.array_equal(sim.done, before[4])
