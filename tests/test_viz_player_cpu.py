"""The adder-viz player on the CPU: (1) the literal Python restatement of `consume` (tests/viz_player_oracle.py) against
the committed C checker driven through the same loop; (2) the product's pop schedule (adder_viz_schedule_host: the
function the schedule kernel runs) and its content rule against the restatement, on the seeded set and exhaustively
on every interleaving of short per-unit sequences; (3) a census of what the seeded set reaches, so that none of this
passes vacuously.

Census of the committed seeds (printed by test_census with -s), recorded in CENSUS below: 43 streams, 3 336 frames
popped before the drain of which 1 746 (52 %) hold a None, 7 518 late-dropped fills, 640 natural and 69 forced `consume`
returns, 126 events that forced a row while another row stalled the pop, a longest cascade of 247 frames, 35 first calls
that ended with the period open, up to 174 flushed frames in one finish, 1 381 AbsoluteT events from a unit's past, 428 of
them from a unit more than buffer_limit frames ahead.  The assertion is the issue's: each kind at least once, at least a
third of the frames popped before the drain hold a None.
"""
import itertools

import numpy as np
import pytest

import viz_player_cases as K
from viz_player_oracle import VizRestatement, unit_chain, some_masks_from_schedule, DELTA_T, ABSOLUTE_T, EVENT_DTYPE

# what the committed seeds give (test_census compares, so a change of the generator shows)
CENSUS = dict(streams=43, before_drain=3336, with_none=1746, late_drops=7518, forced=69, natural=640, stalls=126,
              cascade=247, flushed=174, open_calls=35, past=1381, past_would_force=428)


@pytest.fixture(scope="module")
def seeded():
    """every stream once: (name, cfg, events, restatement after feed in two calls + finish, frames before the drain)"""
    out = []
    for name, cfg, ev in K.seeded_set():
        r = VizRestatement(**cfg)
        cut = len(ev) // 2
        r.feed(ev[:cut])
        open_after_first = r.n_ingested > 0 and (not r.popped or r.popped[-1][0] != r.n_ingested - 1)
        r.feed(ev[cut:])
        before_drain = len(r.popped)
        r.finish()
        out.append((name, cfg, ev, r, before_drain, open_after_first))
    return out


def test_restatement_matches_the_c_checker(seeded):
    """pop positions and popped-form bytes of every frame, the drain included"""
    for name, cfg, ev, r, _, _ in seeded:
        want = K.c_checker_frames(ev, cfg)
        assert [p for p, _ in want] == [p[0] for p in r.popped], name
        for k, (_, b) in enumerate(want):
            assert np.array_equal(b, r.popped[k][1]), (name, k)


def _chain(cfg, ev):
    r = VizRestatement(**cfg)
    return unit_chain(ev, cfg["width"], cfg["channels"], tpf=r.tpf, ref_interval=cfg["ref_interval"], abs_t=r.abs_t,
                      round_up=r.round_up)


def _check_schedule(name, cfg, ev, r, before_drain):
    from adder_amd import viz_player as V
    row, frm, to, last, unit = _chain(cfg, ev)
    n_units = cfg["width"] * cfg["height"] * cfg["channels"]
    for finish in (False, True):
        pops, flushed = V.schedule_host(row, frm, to, last, cfg["height"], cfg["width"] * cfg["channels"],
                                        cfg["buffer_limit"], finish=finish)
        want = r.popped if finish else r.popped[:before_drain]
        assert [p[0] for p in want] == list(pops), (name, finish)
        some = some_masks_from_schedule(pops, frm, to, unit, n_units)
        for k, (_, _, wsome, _) in enumerate(want):
            if flushed[k]:
                assert wsome.all(), (name, k)  # a flushed frame has no None left
            else:
                assert np.array_equal(some[k], wsome), (name, k)
        assert int(flushed.sum()) == (r.flushes if finish else 0), name


def test_schedule_host_matches_the_restatement(seeded):
    for name, cfg, ev, r, before_drain, _ in seeded:
        _check_schedule(name, cfg, ev, r, before_drain)


@pytest.mark.parametrize("limit", [1, 2])
def test_schedule_host_on_every_interleaving(limit):
    """a 2x2 plane, per unit a short sequence of DeltaT steps (in frames): every order in which the four sequences can
    interleave"""
    per_unit = [[1, 1], [3], [1, 4], [2, 1]]  # frames each event advances its unit by
    labels = [u for u, seq in enumerate(per_unit) for _ in seq]
    cfg = K.base_cfg(2, 2, 1, buffer_limit=limit)
    seen = 0
    for order in sorted(set(itertools.permutations(labels))):
        nxt = [0] * 4
        ev = np.zeros(len(order), EVENT_DTYPE)
        for i, u in enumerate(order):
            ev[i] = (u % 2, u // 2, 0xFF, 3, 0, per_unit[u][nxt[u]] * 255)
            nxt[u] += 1
        r = VizRestatement(**cfg)
        r.feed(ev)
        before = len(r.popped)
        r.finish()
        _check_schedule(str(order), cfg, ev, r, before)
        seen += 1
    assert seen == 630  # 7! / (2! 1! 2! 2!)


def test_census(seeded):
    tot = dict(streams=len(seeded), before_drain=0, with_none=0, late_drops=0, forced=0, natural=0, stalls=0,
               cascade=0, flushed=0, open_calls=0, past=0, past_would_force=0)
    for name, cfg, ev, r, before_drain, open_after_first in seeded:
        tot["before_drain"] += before_drain
        tot["with_none"] += sum(1 for p in r.popped[:before_drain] if not p[2].all())
        tot["late_drops"] += r.late_drops
        tot["forced"] += r.forced_pops
        tot["natural"] += r.natural_pops
        tot["stalls"] += r.stalls
        tot["cascade"] = max(tot["cascade"], r.longest_cascade)
        tot["flushed"] = max(tot["flushed"], r.flushes)
        tot["open_calls"] += int(open_after_first)
        tot["past"] += r.past_events
        tot["past_would_force"] += r.past_would_force
    print("census:", tot)
    assert tot["natural"] >= 1 and tot["forced"] >= 1 and tot["cascade"] >= 3 and tot["late_drops"] >= 1
    assert tot["stalls"] >= 1 and tot["open_calls"] >= 1 and tot["flushed"] >= 2
    assert tot["past"] >= 1 and tot["past_would_force"] >= 1
    assert 3 * tot["with_none"] >= tot["before_drain"] > 0
    assert {k: tot[k] for k in CENSUS} == CENSUS


def test_the_c_example_compiles_with_warnings_as_errors(tmp_path):
    import os
    import subprocess
    import adder_amd
    adder_amd.load()  # makes sure the library exists
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "adder-codec-rs_amd")
    exe = str(tmp_path / "adder_viz_play")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "adder_viz_play.c"), "-L", lib, "-ladder_hip",
                           "-Wl,-rpath," + lib, "-o", exe])
    assert os.path.exists(exe)


def test_refusals_of_the_host_schedule():
    from adder_amd import viz_player as V
    with pytest.raises(ValueError):
        V.schedule_host([0], [-1], [0], [0], rows=1, row_units=1, buffer_limit=0)  # limit 0: the loop never ends
    with pytest.raises(ValueError):
        V.schedule_host([1], [-1], [0], [0], rows=1, row_units=1, buffer_limit=2)  # a row outside the plane
    pops, flushed = V.schedule_host([], [], [], [], rows=2, row_units=3, buffer_limit=2, finish=True)
    assert len(pops) == 0 and len(flushed) == 0
