"""adder_hip_integrate_sparse[_device] (csrc/adder_sparse.hip, cont_step) against the oracle on the lists of
tests/sparse_cases.py: events, their count and running_intensities(), byte for byte.  What every list reaches is
asserted on the CPU (test_sparse_edges_cpu.py, which also holds the references used here)."""
import numpy as np
import pytest

from oracle import oracle as O
import sim_py
import sparse_cases as SC
from test_sparse_edges_cpu import (change_quality, oracle_for, oracle_run, oracle_run_after_reset, sim_for, start_frame)

pytestmark = pytest.mark.gpu


def _hip():
    import adder_amd
    return adder_amd


def hip_for(case, max_depth=None):
    A = _hip()
    hv = A.HipVideo(case.W, case.height, case.Cn, row_begin=case.row_begin, row_end=case.row_begin + case.rows,
                    time_mode=case.time_mode, multi_mode=case.multi_mode, ref_time=SC.REF_TIME,
                    delta_t_max=case.delta_t_max, max_depth=case.max_depth if max_depth is None else max_depth, pixel_mode=1)
    hv.set_crf_parameters(*case.crf)
    hv.enable_running_intensities(True)
    return hv


def run_starts(case, hv):
    for a in oracle_run(case)[0]:
        b = hv.integrate_matrix(start_frame(case), time_spanned=float(SC.REF_TIME))
        assert np.array_equal(a, b)


def same_call(hv, st, want, exact_cap=False):
    got = hv.integrate_sparse(st, out_cap=len(want) if exact_cap else None)
    assert hv.last_required == len(want)
    assert len(got) == len(want) and np.array_equal(got, want)


def same_plane(hv, want_plane):
    assert np.array_equal(hv.running_intensities().reshape(-1), want_plane)


def refused(code):
    return pytest.raises(_hip().AdderHipError, match=f"adder_hip error {code}:")


@pytest.mark.parametrize("case", SC.PARITY_CASES + SC.WORKSPACE_CASES, ids=repr)
def test_product_equals_oracle(case):
    _, want, want_plane = oracle_run(case)
    hv = hip_for(case)
    run_starts(case, hv)
    for k, st in enumerate(case.calls):
        if case.quality_change and case.quality_change[0] == k:
            change_quality(case, hv)
        same_call(hv, st, want[k], case.exact_cap)
    same_plane(hv, want_plane)


@pytest.mark.parametrize("case", SC.REFUSAL_CASES, ids=repr)
def test_step_outside_the_band_is_refused(case):
    A = _hip()
    bad, good = case.calls
    _, want, want_plane = oracle_run_after_reset(case)
    hv = hip_for(case)
    with refused(A.E_BAD_PARAMS):
        hv.integrate_sparse(bad)
    with refused(A.E_POISONED):
        hv.integrate_sparse(good)
    hv.reset()
    same_call(hv, good, want)
    same_plane(hv, want_plane)


def _device_steps(st, stream=None):
    import torch
    host = torch.from_numpy(np.ascontiguousarray(st).view(np.uint8).copy())
    if stream is None:
        return host.to("cuda:0")
    with torch.cuda.stream(stream):
        return host.to("cuda:0")


def _events(d_out, n):
    import torch
    torch.cuda.synchronize()
    return np.frombuffer(d_out[: 12 * n].cpu().numpy().tobytes(), dtype=_hip().EVENT_DTYPE)


def test_out_capacity_through_the_device_form():
    """out_cap = total - 1: E_OUT_CAPACITY, last_required = total, nothing behind out_cap written, poisoned; reset
    restores, and out_cap = total passes."""
    import torch
    A = _hip()
    case = next(c for c in SC.PARITY_CASES if c.name == "grid_n1025")
    _, want, _ = oracle_run(case)
    st, want0 = case.calls[0], want[0]
    total, guard = len(want0), 64
    assert total > 256
    hv = hip_for(case)
    run_starts(case, hv)
    d_steps = _device_steps(st)
    d_out = torch.full(((total + guard) * 12,), 0xA5, dtype=torch.uint8, device="cuda:0")
    with refused(A.E_OUT_CAPACITY):
        hv.integrate_sparse_device(d_steps, len(st), d_out, total - 1)
    assert hv.last_required == total
    torch.cuda.synchronize()
    assert bool((d_out[(total - 1) * 12:] == 0xA5).all())
    assert np.array_equal(_events(d_out, total - 1), want0[: total - 1])
    with refused(A.E_POISONED):
        hv.integrate_sparse_device(d_steps, len(st), d_out, total)
    hv.reset()
    run_starts(case, hv)
    d_out.fill_(0xA5)
    assert hv.integrate_sparse_device(d_steps, len(st), d_out, total) == total == hv.last_required
    assert np.array_equal(_events(d_out, total), want0)
    assert bool((d_out[total * 12:] == 0xA5).all())


def test_no_steps_is_no_call():
    """n == 0 returns nothing and leaves the context dense: a frame afterwards is accepted and equals the oracle."""
    import torch
    case = next(c for c in SC.PARITY_CASES if c.name == "grid_n257")
    hv, ov = hip_for(case), oracle_for(case)
    assert len(hv.integrate_sparse(np.zeros(0, O.SPARSE_STEP_DTYPE))) == 0 and hv.last_required == 0
    d_out = torch.zeros(12, dtype=torch.uint8, device="cuda:0")
    assert hv.integrate_sparse_device(None, 0, d_out, 1) == 0
    frame = np.random.default_rng(3).integers(0, 256, (case.rows, case.W, case.Cn)).astype(np.uint8)
    for _ in range(2):
        assert np.array_equal(hv.integrate_matrix(frame, time_spanned=20.0), ov.integrate_matrix(frame, time_spanned=20.0))
    st = case.calls[0]
    assert np.array_equal(hv.integrate_sparse(st), ov.integrate_sparse(st))
    with pytest.raises(_hip().AdderHipError, match="dense frames after sparse"):
        hv.integrate_matrix(frame, time_spanned=20.0)


def test_device_form_alternating_with_the_host_form():
    """Steps and events in torch tensors: on a stream of the caller's, on the context's own (stream=None), and the host
    form in between on the same context -- equal to a context that only used the host form, and to the oracle."""
    import torch
    case = next(c for c in SC.PARITY_CASES if c.name == "run_crosses_block")
    _, want, want_plane = oracle_run(case)
    hv, host_only = hip_for(case), hip_for(case)
    run_starts(case, hv)
    run_starts(case, host_only)
    side = torch.cuda.Stream()
    for k, st in enumerate(case.calls + [case.calls[1]]):
        ref = host_only.integrate_sparse(st)
        if k < len(want):
            assert np.array_equal(ref, want[k])
        if k == 1:
            got = hv.integrate_sparse(st)
        else:
            stream = side if k in (0, 3) else None
            d_steps = _device_steps(st, stream)
            d_out = torch.empty(max(len(ref), 1) * 12, dtype=torch.uint8, device="cuda:0")
            n = hv.integrate_sparse_device(d_steps, len(st), d_out, len(ref), stream=stream.cuda_stream if stream else None)
            assert n == len(ref)
            got = _events(d_out, n)
        assert np.array_equal(got, ref), k
    assert np.array_equal(hv.running_intensities(), host_only.running_intensities())


@pytest.mark.parametrize("case", SC.DEPTH_CASES, ids=repr)
def test_depth_boundary(case):
    """max_depth = P equals the oracle; P - 1 and 1 give E_ARENA_DEPTH, poison the context, and reset restores it.
    The step that overflows is followed by more steps of its pixel in the same call, which the run walk goes through:
    first the list must come clean out of the sim, whose node accessor checks its bounds."""
    A = _hip()
    st = case.calls[0]
    for depth in (1, case.P - 1, case.P):
        rc, _ = sim_for(case, depth).integrate_sparse(st)
        assert rc != sim_py.NODE_OUT_OF_RANGE and rc == (0 if depth == case.P else -5), (depth, rc)
    _, want, want_plane = oracle_run(case)
    hv = hip_for(case, case.P)
    same_call(hv, st, want[0])
    same_plane(hv, want_plane)
    for depth in (case.P - 1, 1):
        hv = hip_for(case, depth)
        with refused(A.E_ARENA_DEPTH):
            hv.integrate_sparse(st)
        with refused(A.E_POISONED):
            hv.integrate_sparse(st[:1])
        hv.reset()
        head = st[: case.overflow_at[depth]]  # the steps in front of the first overflow fit this depth
        ov = oracle_for(case)
        same_call(hv, head, ov.integrate_sparse(head))
        same_plane(hv, ov.running_intensities().reshape(-1))
