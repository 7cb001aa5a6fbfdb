"""The part of a push the Prophesee and the DAVIS source share (csrc/adder_chain.hip: the pair sort with its copy-back,
the count scan with its total, the two-slot compaction; csrc/adder_source_util.hpp: the scratch that grows with the
pushes), through the two public APIs at the smallest shapes where it can go wrong.  Everything is compared bit for bit
with the restatements (prophesee_oracle, davis_oracle), the sources' end state from pixel_state() included.

Pinned elsewhere and not repeated: a refused capacity (test_gpu_prophesee.test_capacity_refusal_leaves_state_unchanged,
test_gpu_davis.test_refused_push_changes_nothing), the device forms of the DAVIS push
(test_gpu_davis.test_device_and_host_push_forms_agree), cuts inside a pixel's run
(test_gpu_chain_arms.test_prophesee_case_whole_and_split) and a DAVIS list of held and new events past one block
(davis_cases' "counts": lists of 512 and 1026 events)."""
import functools

import numpy as np
import pytest

import davis_cases as DC
import davis_oracle as DO
import prophesee_oracle as PR
from adder_amd import _native as N
from adder_amd import davis as D
from adder_amd import prophesee as P
from test_gpu_davis import check_state, push
from test_gpu_prophesee import run_lib, same

pytestmark = pytest.mark.gpu

V = PR.VIEW_INTERVAL
# width x height: 8, 512 and 89960 pixels take 4, 10 and 17 key bits, so the radix sort makes a different number of
# passes and its result ends in the first or in the second pair of buffers
PLANES = [(2, 4), (32, 16), (346, 260)]
# a block is 256 lanes: one record, a block less one, a block, a block and one, more than two blocks and a part
COUNTS = [1, 255, 256, 257, 700]
REF_TIME, CRF = 20, 3


@pytest.fixture(autouse=True)
def _start_up_frames_without_a_captured_graph(monkeypatch):
    """As tests/test_gpu_chain_arms.py: the code under test takes no graph, and the many short-lived contexts of this
    module should not each leave a captured one behind."""
    monkeypatch.setenv("ADDER_HIP_NO_GRAPH", "1")


# ---- Prophesee ----------------------------------------------------------------------------------------------------

def group(rng, W, H, n, t0):
    """n records that are exactly one group when the group starts at t0: n - 1 inside the window, in camera order, on
    a few hot pixels and the rest of the plane, the first on the last pixel; the n-th one tick past the window, on the
    last pixel too.  -> (records, the next group's start)."""
    units = W * H
    t = np.append(np.sort(rng.integers(t0 + 1, t0 + V + 1, n - 1)), t0 + V + 1)
    hot = rng.integers(0, units, 3)
    px = np.where(rng.random(n) < 0.4, hot[rng.integers(0, 3, n)], rng.integers(0, units, n))
    px[0] = px[-1] = units - 1
    return P.records(t, px % W, px // W, rng.integers(0, 2, n)), t0 + V + 1


def tail(t):
    """One record a tick after everything: it opens a group that is dropped, and keeps end_events' assert quiet."""
    return P.records([t + 1], [0], [0], [1])


@functools.lru_cache(maxsize=None)
def pph_want(W, H, sizes):
    """Groups of `sizes` records one after the other and the tail -> (records, oracle events, oracle after the run)."""
    rng = np.random.default_rng(1000 * W + sum(sizes))
    parts, t0 = [], 2
    for n in sizes:
        g, t0 = group(rng, W, H, n, t0)
        parts.append(g)
    recs = np.concatenate(parts + [tail(t0)])
    src = PR.Prophesee(W, H, REF_TIME, CRF)
    want = src.run(PR.decode_body(recs.tobytes()))
    for a in (recs, want):
        a.setflags(write=False)
    return recs, want, src


def pph_check(got, pr, want, src):
    assert same(got, want)
    t, ln = pr.pixel_state()
    assert np.array_equal(t.reshape(-1), np.array(src.last_t, np.uint32))
    assert np.array_equal(ln.reshape(-1).view(np.uint64), np.array(src.last_ln, np.float64).view(np.uint64))
    assert np.array_equal(pr.running_intensities(), src.running_intensities())


@pytest.mark.parametrize("W,H", PLANES)
def test_prophesee_planes(W, H):
    recs, want, src = pph_want(W, H, (700,))
    pph_check(*run_lib(recs, W, H, REF_TIME, CRF, device=True), want, src)


@pytest.mark.parametrize("n", COUNTS)
def test_prophesee_record_counts(n):
    W, H = 32, 16
    recs, want, src = pph_want(W, H, (n,))
    pr = P.HipProphesee(W, H, REF_TIME, CRF)
    out = [pr.start(), pr.push(recs)]
    assert pr.state()["open_records"] == 1  # the chain ran on exactly n records: the tail alone stays open
    out.append(pr.finish())
    pph_check(np.concatenate(out), pr, want, src)


def test_prophesee_record_outside_the_plane_at_a_block_edge():
    W, H, k = 32, 16, 255  # the last lane of the first block, of 257 records
    recs, want, src = pph_want(W, H, (257,))
    bad = recs.copy()
    bad[k] = P.records([int(recs["t"][k])], [W], [0], [1])[0]
    pr = P.HipProphesee(W, H, REF_TIME, CRF)
    out = [pr.start()]
    before, (t0, ln0) = pr.state(), pr.pixel_state()
    with pytest.raises(N.AdderHipError) as ei:
        pr.push(bad)
    assert ei.value.code == P.E_BAD_RECORD and ei.value.index == k == pr.bad_index and pr.state() == before
    t1, ln1 = pr.pixel_state()
    assert np.array_equal(t0, t1) and np.array_equal(ln0.view(np.uint64), ln1.view(np.uint64))
    out += [pr.push(recs), pr.finish()]  # nothing changed: the good stream goes through as on a fresh context
    pph_check(np.concatenate(out), pr, want, src)


@pytest.mark.parametrize("device", [False, True])
def test_prophesee_scratch_grows_and_is_reused(device):
    """Groups of 1, 600 and 1 records, a push each: the scratch is made for one record, replaced for 600 (the device
    form first sizes it for the push's records, to read their t), then used again for one."""
    W, H = 32, 16
    recs, want, src = pph_want(W, H, (1, 600, 1))
    got, pr = run_lib(recs, W, H, REF_TIME, CRF, splits=[1, 601, 602], device=device)
    pph_check(got, pr, want, src)


def test_prophesee_group_split_across_two_pushes():
    """The first push leaves 300 open records and makes nothing; the second closes the group: every kernel of the
    chain then runs on the open group's buffer, holding the records of both."""
    W, H = 32, 16
    recs, want, src = pph_want(W, H, (600,))
    pr = P.HipProphesee(W, H, REF_TIME, CRF)
    out = [pr.start(), pr.push(recs[:300])]
    assert len(out[1]) == 0 and pr.state()["open_records"] == 300
    out.append(pr.push(recs[300:]))
    assert pr.state()["open_records"] == 1
    out.append(pr.finish())
    pph_check(np.concatenate(out), pr, want, src)


# ---- DAVIS --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def davis_want(W, H, n_before, n_after):
    """RawDavis packets with these `before` / `after` counts; the last `before` event of each on the last pixel
    -> (case, oracle's push results, oracle's finish events)."""
    rng = np.random.default_rng(2000 * W + sum(n_before) + sum(n_after))
    packets = DC._packets(rng, W, H, len(n_before), list(n_before), list(n_after), hot=rng.integers(0, W * H, 3))
    for pk in packets:
        if len(pk["before"]):
            pk["before"]["x"][-1], pk["before"]["y"][-1] = W - 1, H - 1
    case = DC._case(f"chain_{W}x{H}", W, H, DO.RAW_DAVIS, packets, crf=2)
    res, fin, _ = DO.run(packets, W, H, DO.RAW_DAVIS, tps=case["tps"], ref_time=case["ref_time"], dtm=case["dtm"], crf=2)
    return case, res, fin


def davis_make(case):
    return D.HipDavis(case["W"], case["H"], case["mode"], case["tps"], case["ref_time"], case["dtm"], crf=case["crf"])


def davis_run(dv, case, res, fin, first=0):
    for pk, want in zip(case["packets"][first:], res[first:]):
        got = push(dv, pk)
        assert len(got) == len(want["events"]) and got.tobytes() == want["events"].tobytes()
        check_state(dv, want)
    got = dv.finish()
    assert len(got) == len(fin) and got.tobytes() == fin.tobytes()
    dv.close()


@pytest.mark.parametrize("W,H", PLANES)
def test_davis_planes(W, H):
    # the second packet's list is the 450 held events and 250 new ones
    case, res, fin = davis_want(W, H, (300, 250), (450, 0))
    davis_run(davis_make(case), case, res, fin)


@pytest.mark.parametrize("n", COUNTS)
def test_davis_list_counts(n):
    # no `after` events are ever held, so the second packet's list is its n `before` events (a context's first packet
    # makes no events in the oracle either: its steps show in the state alone)
    case, res, fin = davis_want(32, 16, (0, n), (0, 0))
    assert len(res[1]["events"]) > 32 * 16
    davis_run(davis_make(case), case, res, fin)


def test_davis_event_outside_the_plane_at_a_block_edge():
    W, H, k = 32, 16, 256  # the first lane of the second block, of 257 events
    case, res, fin = davis_want(W, H, (0, 257), (0, 0))
    pk = dict(case["packets"][1])
    pk["before"] = pk["before"].copy()
    pk["before"]["x"][k] = W
    dv = davis_make(case)
    push(dv, case["packets"][0])
    ts0, ln0 = dv.pixel_state()
    with pytest.raises(N.AdderHipError) as ei:
        push(dv, pk)
    assert ei.value.code == D.E_BAD_EVENT and ei.value.index == k == dv.bad_index
    ts1, ln1 = dv.pixel_state()
    assert np.array_equal(ts0, ts1) and np.array_equal(ln0.view(np.uint64), ln1.view(np.uint64))
    davis_run(dv, case, res, fin, first=1)  # nothing changed: the good packet goes through as if never refused


def test_davis_scratch_grows_and_is_reused():
    """Lists of 0, 1, 600 and 1 events on one context.  The first push has no list at all -- no held events, an empty
    `before` -- and still scans its plane for the gaps, so the scan's temp must be there before any list scratch is."""
    case, res, fin = davis_want(32, 16, (0, 1, 600, 1), (0, 0, 0, 0))
    assert len(case["packets"][0]["before"]) == 0
    davis_run(davis_make(case), case, res, fin)
