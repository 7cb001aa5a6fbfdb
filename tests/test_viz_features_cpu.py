"""Feature detection in the adder-viz player on the CPU: (1) the hand-derived cases (tests/viz_features_cases.py) on the
literal restatement (tests/viz_features_oracle.py); (2) that restatement against the two it extends, where their
domains overlap; (3) the product's decomposition -- the period-start mask, W_i, the stamp cursor and the running-frame
rule, compiled for the host -- against the restatement, on the seeded streams and exhaustively on every interleaving of
short per-unit sequences with synthetic corner marks; (4) a census of what the seeded streams reach.

Census of the committed seeds (test_census prints it with -s), recorded in CENSUS below: 32 streams (four planes, DeltaT
and AbsoluteT, limits 1, 2, 60 and None), 4 683 features of which 372 come from an event that was dropped as late for a
frame and 1 766 are filed at an index above 0; 5 corners not tested only because their event opened a period; 39 788
(unit, frame) pairs where a cross was kept across a None and 26 346 where a Some overwrote one; intervals with features
popped by the first pop of a forced return (86), by a later pop of one loop (63) and by finish (140).
"""
import itertools

import numpy as np
import pytest

import viz_features_cases as FC
import viz_player_cases as K
from framer_features_oracle import Restatement, DELTA_T, ABSOLUTE_T, EVENT_DTYPE
from viz_features_oracle import VizFeatureRestatement
from viz_player_oracle import VizRestatement, unit_chain

# what the committed seeds give (test_census compares, so a change of the generator shows)
CENSUS = dict(streams=32, features=4683, late_features=372, suppressed=5, cross_kept=39788, cross_overwritten=26346,
              iv_forced=86, iv_cascade=63, iv_finish=140, idx_above_0=1766)


@pytest.mark.parametrize("case", FC.CASES, ids=[c["name"] for c in FC.CASES])
def test_known_answers_on_the_restatement(case):
    FC.check(case, FC.run(FC.RestatementImpl(case["cfg"]), case["ops"]))


seeded = FC.seeded

SMALL = [(n, tm, lim) for n in ("9x8", "12x9rgb") for tm in (DELTA_T, ABSOLUTE_T) for lim in FC.LIMITS]
ALL = [(n, tm, lim) for n in FC.SEEDED for tm in (DELTA_T, ABSOLUTE_T) for lim in FC.LIMITS]


@pytest.mark.parametrize("name,time_mode,limit", SMALL)
def test_popped_frames_are_the_viz_restatements(name, time_mode, limit):
    """detection changes no popped frame, and no running frame outside the crosses"""
    cfg, ev, r, _, _ = seeded(name, time_mode, limit)
    v = VizRestatement(**cfg)
    v.feed(ev)
    v.finish()
    assert len(v.popped) == len(r.popped) == len(r.intervals)
    for a, b in zip(v.popped, r.popped):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name,time_mode", [(n, tm) for n in ("9x8", "12x9rgb") for tm in (DELTA_T, ABSOLUTE_T)])
def test_without_limit_and_per_consume_reset_it_is_the_framers_restatement(name, time_mode):
    cfg = FC.seeded_cfg(name, time_mode, None)
    ev = FC.seeded_stream(name, time_mode)[:1500]
    a = VizFeatureRestatement(per_consume_reset=False, **cfg)
    a.detect_features(True)
    f = Restatement(cfg["width"], cfg["height"], cfg["channels"], tps=cfg["tps"], ref_interval=cfg["ref_interval"],
                    delta_t_max=cfg["delta_t_max"], output_fps=cfg["output_fps"], codec_version=cfg["codec_version"],
                    time_mode=cfg["time_mode"], source_camera=cfg["source_camera"])
    f.detect_features(True)
    feats_a, feats_f, iv_f = [], [], []
    for i in range(len(ev)):
        popped = a.feed(ev[i:i + 1])
        feats_a += [tuple(int(v) for v in r) for r in a.last_features.tolist()]
        feats_f += [tuple(int(v) for v in r) for r in f.ingest(ev[i:i + 1], index_base=i).tolist()]
        for p in popped:  # the player: write_frame_bytes, then pop_features
            assert np.array_equal(np.frombuffer(f.write_frame_bytes(), np.uint8), p[1])
            end_ts, xy = f.pop_features()
            iv_f.append((int(end_ts), [tuple(int(v) for v in q) for q in xy]))
    assert feats_a == feats_f and len(feats_a) >= 10
    assert a.intervals == iv_f and sum(len(xy) for _, xy in iv_f) >= 5
    assert np.array_equal(a.running_intensities, f.running_intensities())


# ---- the product's decomposition on the host ----------------------------------------------------------------------

def decomposed(cfg, ev, marks, finish=True, paint=True):
    """features, intervals and running frames from the product's pieces: the unit chain, adder_viz_schedule_host,
    adder_viz_features_host (period-start mask, W_i), the host's filing in event / pop order, the stamps and
    adder_viz_overlay_host -- with the popped frames' Some / values taken from VizRestatement."""
    from adder_amd import viz_player as V
    v = VizRestatement(**cfg)
    row, frm, to, last, unit = unit_chain(ev, cfg["width"], cfg["channels"], tpf=v.tpf, ref_interval=cfg["ref_interval"],
                                          abs_t=v.abs_t, round_up=v.round_up)
    pops, _ = V.schedule_host(row, frm, to, last, cfg["height"], cfg["width"] * cfg["channels"], cfg["buffer_limit"],
                              finish=finish)
    marks = np.array(marks, np.uint8)
    marks[:1] = 0  # a fresh context carries no last event: the candidate test never marks the stream's first event
    kept, w = V.features_host(pops, marks)
    v.feed(ev)
    if finish:
        v.finish()
    assert [p[0] for p in v.popped] == list(pops)
    dq = Restatement(cfg["width"], cfg["height"], cfg["channels"], tps=cfg["tps"], ref_interval=cfg["ref_interval"],
                     delta_t_max=cfg["delta_t_max"], output_fps=cfg["output_fps"])
    feats, intervals, stamps = [], [], []
    nxt = 0
    idx = [i for i in range(len(ev)) if kept[i]]

    def file_until(last_index):
        nonlocal nxt
        while nxt < len(idx) and idx[nxt] <= last_index:
            i = idx[nxt]
            dq.frames_written = int(w[i])
            dq._file(int(ev["t"][i]), int(ev["x"][i]), int(ev["y"][i]))
            feats.append((i, int(ev["t"][i]), int(ev["x"][i]), int(ev["y"][i])))
            nxt += 1

    ch, wd = cfg["channels"], cfg["width"]
    for k, p in enumerate(pops):
        file_until(int(p))
        end_ts, xy = dq.pop_features()
        intervals.append((int(end_ts), [tuple(int(q) for q in c) for c in xy]))
        for x, y in intervals[-1][1]:
            for i in range(-2, 3):
                for c in range(ch):
                    stamps.append((((y + i) * wd + x) * ch + c, k))
                    stamps.append(((y * wd + x + i) * ch + c, k))
    file_until(len(ev))
    if not paint:
        return feats, intervals, None, None
    some = np.array([p[2] for p in v.popped], np.uint8).reshape(len(pops), -1)
    val = np.array([p[1] for p in v.popped], np.uint8).reshape(len(pops), -1)
    n_units = cfg["width"] * cfg["height"] * ch
    frames, run = V.overlay_host(some.reshape(len(pops), n_units), val.reshape(len(pops), n_units), stamps,
                                 np.zeros(n_units, np.uint8))
    return feats, intervals, frames, run


class Marked(VizFeatureRestatement):
    """corners by decree: event i is one iff marks[i] (a 2x2 plane has no FAST candidates of its own, and no room for
    a cross: the intervals are kept aside and nothing is painted)"""

    def __init__(self, marks, **cfg):
        super().__init__(**cfg)
        self.marks = marks
        self.true_intervals = []
        self.F._is_feature = lambda x, y, c: bool(self.marks[self.n_ingested - 1])

    def _pop_features(self):
        end_ts, features = super()._pop_features()
        self.true_intervals.append((end_ts, [(int(a), int(b)) for a, b in features]))
        return end_ts, []


@pytest.mark.parametrize("limit", [1, 2, None])
def test_period_start_mask_and_w_on_every_interleaving(limit):
    """the 2x2 plane and per-unit sequences of test_viz_player_cpu's interleavings; every event is a corner by decree,
    then every other one"""
    per_unit = [[1, 1], [3], [1, 4], [2, 1]]
    labels = [u for u, seq in enumerate(per_unit) for _ in seq]
    cfg = K.base_cfg(2, 2, 1, buffer_limit=limit)
    seen = filed = masked = above = 0
    for order in sorted(set(itertools.permutations(labels))):
        nxt = [0] * 4
        ev = np.zeros(len(order), EVENT_DTYPE)
        for i, u in enumerate(order):
            # t differs from event to event (a delta of 255 * frames, minus i: the clock rounds up to the same frame)
            ev[i] = (u % 2, u // 2, 0xFF, 3, 0, per_unit[u][nxt[u]] * 255 - i)
            nxt[u] += 1
        for marks in (np.ones(7, np.uint8), (np.arange(7) % 2 == seen % 2).astype(np.uint8)):
            r = Marked(marks, **cfg)
            r.detect_features(True)
            r.feed(ev)
            feats = [tuple(int(v) for v in f) for f in r.last_features.tolist()]
            r.finish()
            got = decomposed(cfg, ev, marks, paint=False)
            assert got[0] == feats, (order, limit)
            assert got[1] == r.true_intervals, (order, limit)
            filed += len(feats)
            masked += int(marks.sum()) - len(feats)
            above += r.c_idx_above_0
        seen += 1
    # corners were filed, the period-start rule took some away (beyond event 0, which is never tested)
    assert seen == 630 and filed > 0 and masked > 2 * 630
    assert limit is not None or above > 0


def test_running_frame_rule_on_every_short_history():
    """one unit among three, three frames: every combination of Some / None and stamped / not, from every running value;
    against `Some overwrites, None keeps, then the cross wins` written out"""
    from adder_amd import viz_player as V
    for combo in itertools.product(range(4), repeat=3):
        for start in (0, 7):
            some = np.zeros((3, 3), np.uint8)
            val = np.zeros((3, 3), np.uint8)
            stamps, cur, want = [(0, 1), (2, 0), (2, 2)], start, []
            for k, cmb in enumerate(combo):
                some[k, 1], val[k, 1] = cmb & 1, 10 + k
                if cmb & 1:
                    cur = 10 + k
                if cmb & 2:
                    stamps += [(1, k), (1, k)]  # twice: the arms of a cross share its centre
                    cur = 255
                want.append(cur)
            frames, run = V.overlay_host(some, val, stamps, [5, start, 6])
            assert frames[:, 1].tolist() == want and run[1] == cur, combo
            assert frames[:, 0].tolist() == [5, 255, 255] and frames[:, 2].tolist() == [255, 255, 255]


@pytest.mark.parametrize("name,time_mode,limit", SMALL)
def test_host_logic_on_the_seeded_streams(name, time_mode, limit):
    """the corners the restatement found, as marks before the period-start rule: every event that differs in t from its
    predecessor and is a corner on the plane (restated with per_consume_reset off)"""
    cfg, ev, r, _, feats = seeded(name, time_mode, limit)
    free = VizFeatureRestatement(per_consume_reset=False, **cfg)
    free.detect_features(True)
    free.feed(ev)
    marks = np.zeros(len(ev), np.uint8)
    marks[free.last_features["index"].astype(np.int64)] = 1
    got = decomposed(cfg, ev, marks)
    assert got[0] == [tuple(int(v) for v in f) for f in feats.tolist()]
    assert got[1] == r.intervals
    assert np.array_equal(got[2], np.array([p[3] for p in r.popped], np.uint8).reshape(got[2].shape))
    assert np.array_equal(got[3], r.running)


def test_refusals_of_the_host_entries():
    from adder_amd import viz_player as V
    with pytest.raises(ValueError):
        V.features_host([3, 1], [1, 1, 1, 1])  # pops must not decrease
    kept, w = V.features_host([-1, 0, 0, 2], [1, 1, 1, 1, 1], w0=5)
    assert list(kept) == [0, 0, 1, 0, 1] and list(w) == [6, 8, 8, 9, 9]
    frames, run = V.overlay_host([[0, 1], [0, 0]], [[9, 7], [0, 0]], [(1, 0), (1, 0), (0, 1)], [3, 4])
    assert frames.tolist() == [[3, 255], [255, 255]] and run.tolist() == [255, 255]


# ---- census ---------------------------------------------------------------------------------------------------------

def test_census():
    tot = dict(streams=0, features=0, late_features=0, suppressed=0, cross_kept=0, cross_overwritten=0, iv_forced=0,
               iv_cascade=0, iv_finish=0, idx_above_0=0)
    for name, tm, lim in ALL:
        _, _, r, _, feats = seeded(name, tm, lim)
        tot["streams"] += 1
        tot["features"] += len(feats)
        tot["late_features"] += r.c_late_features
        tot["suppressed"] += r.c_suppressed
        tot["cross_kept"] += r.c_cross_kept
        tot["cross_overwritten"] += r.c_cross_overwritten
        tot["iv_forced"] += r.c_iv_forced
        tot["iv_cascade"] += r.c_iv_cascade
        tot["iv_finish"] += r.c_iv_finish
        tot["idx_above_0"] += r.c_idx_above_0
        assert r.broken is None
    print("census:", tot)
    assert all(tot[k] >= 1 for k in tot), tot
    assert tot == CENSUS
