"""tests/sparse_cases.py on the CPU: every case reaches the edge it names, and the device header's flow (tests/cpu_sim,
cont_step with per-unit c_thresh / running_t, the side plane) equals the oracle byte for byte on every list -- events of
every call and the running plane.  The sim's node accessor checks its bounds: no list, at any max_depth, may make
cont_step ask for a node outside the unit's arena.  (The product on these lists: test_gpu_sparse_edges.py.)"""
import numpy as np
import pytest

from oracle import oracle as O
import sim_py
from sim_py import Sim
import sparse_cases as SC


def oracle_for(case):
    ov = O.Video(case.W, case.rows, case.Cn, row_begin=case.row_begin, time_mode=case.time_mode,
                 multi_mode=case.multi_mode, ref_time=SC.REF_TIME, delta_t_max=case.delta_t_max)
    ov.set_pixel_mode(1)
    ov.ensure_capacity(case.max_depth + 3)
    ov.set_crf_parameters(*case.crf)
    return ov


def sim_for(case, max_depth=None):
    sv = Sim(case.W, case.rows, case.Cn, row_begin=case.row_begin, time_mode=case.time_mode, multi_mode=case.multi_mode,
             ref_time=SC.REF_TIME, delta_t_max=case.delta_t_max, max_depth=case.max_depth if max_depth is None else max_depth)
    sv.set_continuous()
    sv.set_crf_parameters(*case.crf)
    return sv


def start_frame(case):
    return np.full((case.rows, case.W, case.Cn), 128, np.uint8)


def change_quality(case, v):
    _, c_max, vel, dtm, base = case.quality_change
    v.set_crf_parameters(c_max, vel)
    v.set_delta_t_max(dtm)
    v.reset_c_thresh(base)


def oracle_run(case):
    """[(events of call k)], running plane: the reference for both test files, computed once per case."""
    if not hasattr(case, "_oracle"):
        ov = oracle_for(case)
        starts = [ov.integrate_matrix(start_frame(case), time_spanned=float(SC.REF_TIME)) for _ in range(case.start_frames)]
        events = []
        for k, st in enumerate(case.calls):
            if case.quality_change and case.quality_change[0] == k:
                change_quality(case, ov)
            events.append(ov.integrate_sparse(st))
        case._oracle = (starts, events, ov.running_intensities().reshape(-1))
        for a in starts + events + [case._oracle[2]]:
            a.setflags(write=False)
    return case._oracle


@pytest.mark.parametrize("case", SC.ALL_CASES, ids=repr)
def test_case_reaches_its_edge(case):
    assert case.reached(), case.edge


@pytest.mark.parametrize("case", SC.PARITY_CASES + SC.WORKSPACE_CASES + SC.DEPTH_CASES, ids=repr)
def test_sim_equals_oracle(case):
    starts, want, want_plane = oracle_run(case)
    sv = sim_for(case)
    for a in starts:
        rc, b = sv.integrate(start_frame(case), float(SC.REF_TIME))
        assert rc == 0 and np.array_equal(a, b)
    total = 0
    for k, st in enumerate(case.calls):
        if case.quality_change and case.quality_change[0] == k:
            change_quality(case, sv)
        rc, b = sv.integrate_sparse(st)
        assert rc == 0, (k, rc)  # (the case's max_depth is enough)
        assert len(b) == len(want[k]) and np.array_equal(b, want[k]), k
        total += len(b)
    assert total > 0
    assert np.array_equal(sv.running_plane(), want_plane)


@pytest.mark.parametrize("case", SC.REFUSAL_CASES, ids=repr)
def test_refusals_agree(case):
    """A list with a step outside the band is refused by both; the list for after reset() equals on fresh contexts."""
    bad, good = case.calls
    ov, sv = oracle_for(case), sim_for(case)
    with pytest.raises(ValueError):
        ov.integrate_sparse(bad)
    assert sv.integrate_sparse(bad)[0] == -1
    starts, want, want_plane = oracle_run_after_reset(case)
    sv = sim_for(case)
    rc, b = sv.integrate_sparse(good)
    assert rc == 0 and np.array_equal(b, want) and len(want) > 0
    assert np.array_equal(sv.running_plane(), want_plane)


def oracle_run_after_reset(case):
    """The refusal cases' second list on a fresh context: (none, events, running plane)."""
    if not hasattr(case, "_oracle_good"):
        ov = oracle_for(case)
        ev = ov.integrate_sparse(case.calls[1])
        case._oracle_good = (None, ev, ov.running_intensities().reshape(-1))
    return case._oracle_good


def test_quality_change_resets_every_units_pair():
    """The sparse arm of reset_c_thresh: without it the fourth call of a quality case differs (the gap this pins)."""
    case = next(c for c in SC.PARITY_CASES if c.quality_change)
    _, want, _ = oracle_run(case)
    sv = sim_for(case)
    for _ in range(case.start_frames):
        sv.integrate(start_frame(case), float(SC.REF_TIME))
    for k in range(3):
        assert np.array_equal(sv.integrate_sparse(case.calls[k])[1], want[k])
    # quality parameters without the reset: the per-unit pairs keep their advanced values, and the events show it
    sv.set_crf_parameters(*case.quality_change[1:3])
    sv.set_delta_t_max(case.quality_change[3])
    rc, b = sv.integrate_sparse(case.calls[3])
    assert rc == 0 and not np.array_equal(b, want[3])


# ------------------------------------------------------------------------------------------------------------------
# the depth boundary
# ------------------------------------------------------------------------------------------------------------------
def first_failing_step(case, depth):
    sv = sim_for(case, depth)
    for i in range(len(case.calls[0])):
        rc, _ = sv.integrate_sparse(case.calls[0][i:i + 1])
        assert rc in (0, -5), (i, rc)
        if rc:
            return i
    return None


@pytest.mark.parametrize("case", SC.DEPTH_CASES, ids=repr)
def test_depth_sweep_stays_inside_the_arena(case):
    """Every max_depth from 1 to P: ARENA_DEPTH (-5) below P, 0 at P, and never a node index outside the arena -- the
    accessor would report NODE_OUT_OF_RANGE instead of touching it.  Before cont_step refused to step an emptied arena
    these lists gave that code at max_depth 1 (and 1..5 at delta_t_max 160): index 0xffffffff."""
    st = case.calls[0]
    for depth in range(1, case.P + 1):
        rc, ev = sim_for(case, depth).integrate_sparse(st)
        assert rc != sim_py.NODE_OUT_OF_RANGE, depth
        assert rc == (0 if depth == case.P else -5), (depth, rc)
    rc, ev = sim_for(case, case.P + 1).integrate_sparse(st)
    assert rc == 0 and np.array_equal(ev, oracle_run(case)[1][0])
    for depth, step in case.overflow_at.items():  # the recorded first overflow, which the reach predicate builds on
        assert first_failing_step(case, depth) == step, depth


def test_depth_sweep_of_random_lists():
    """The same property on lists nobody chose: 8x4 plane, every flag, both multi modes, three delta_t_max."""
    case = SC.DEPTH_CASES[0]
    rng = np.random.default_rng(4242)
    failed = 0
    for dtm in (160, 1280, 81920):
        for mm in (O.NORMAL, O.COLLAPSE):
            st = case.rand(rng, 3000, hot=0.5)
            for depth in range(1, 14):
                sv = Sim(8, 4, 1, time_mode=O.DELTA_T, multi_mode=mm, ref_time=SC.REF_TIME, delta_t_max=dtm, max_depth=depth)
                sv.set_continuous()
                rc, _ = sv.integrate_sparse(st)
                assert rc in (0, -5), (dtm, mm, depth, rc, sv.node_oob_index)
                failed += rc == -5
    assert failed > 30


def test_dense_continuous_frames_stay_inside_the_arena():
    """adder_cont_kernel steps a unit once per frame and a batch runs several frames without a host check in between.
    A full step cannot empty an arena, though: after a flush the root always fires (intensity >= 2^get_d(intensity))
    and gets its child, so the childless node of an overflow never becomes the root of a one-node arena.  Checked here
    with the same accessor, frames that hold and change, zeros included, at depths that overflow at once."""
    rng = np.random.default_rng(77)
    T, failed = 100, 0
    clip = np.zeros((T, 4, 8, 1), np.uint8)
    for y in range(4):
        for x in range(8):
            k = 0
            while k < T:
                hold = int(rng.integers(1, 13))
                clip[k:k + hold, y, x, 0] = rng.choice(np.array([0, 0, 1, 2, 40, 255]))
                k += hold
    for mm in (O.NORMAL, O.COLLAPSE):
        for dtm in (255, 1020, 7650):
            for depth in (1, 2, 3):
                sv = Sim(8, 4, 1, time_mode=O.DELTA_T, multi_mode=mm, ref_time=255, delta_t_max=dtm, max_depth=depth)
                sv.set_continuous()
                sv.set_crf_parameters(0, 10)
                sv.reset_c_thresh(0)
                rcs = [sv.integrate(clip[k], 255.0 if k % 5 else 510.0)[0] for k in range(T)]
                assert set(rcs) <= {0, -5}, (mm, dtm, depth, sv.node_oob_index)
                failed += -5 in rcs
    assert failed >= 12
