"""Every arm of the Prophesee and DVS chain kernels on the device (pph_walk_kernel / pph_end_kernel in
csrc/adder_prophesee.hip, dvs_ln_kernel / dvs_walk_kernel in csrc/adder_dvs.hip): the constructed cases of
tests/chain_arm_cases.py -- tests/test_chain_arms_cpu.py holds them to their arms -- byte for byte against the
restatements, whole and split inside the constructed runs, with a bad record or event inside a run.  No tolerances:
everything compared is integers, bytes or bit patterns of doubles."""
import functools

import numpy as np
import pytest

import adder_stream_np as S
import chain_arm_cases as K
import dvs_oracle as DR
import prophesee_oracle as PR
from adder_amd import _native as N
from adder_amd import prophesee as P
from test_gpu_dvs import as_list
from test_gpu_prophesee import run_lib, same

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _start_up_frames_without_a_captured_graph(monkeypatch):
    """These tests open well over a hundred Prophesee contexts, each with an inner dense context whose two start-up
    frames would instantiate a captured graph that dies with the context.  This HIP runtime is known to crash in a
    later hipGraphLaunch of another instance once many instances have been destroyed in the process
    (csrc/adder_hip_ctx.hpp, retired_execs), so the contexts of this module launch their start-up frames eagerly
    (read at create): the chain kernels under test and the sparse integrator take no graph either way, and the
    start-up frames through their graph are tests/test_gpu_prophesee.py's."""
    monkeypatch.setenv("ADDER_HIP_NO_GRAPH", "1")


# ---- Prophesee ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pph(kind, ref_time, crf):
    """The case, the oracle's events (read-only) and the oracle after the run."""
    case = K.prophesee_case(kind, ref_time)
    src = PR.Prophesee(case["W"], case["H"], ref_time, crf)
    want = src.run(PR.decode_body(case["recs"].tobytes()))
    want.setflags(write=False)
    return case, want, src


def pph_check(got, pr, want, src, n_records):
    assert same(got, want)
    assert np.array_equal(pr.running_intensities(), src.running_intensities())
    st = pr.state()
    assert st["running_t"] == src.running_t and st["records_pushed"] == n_records
    t, ln = pr.pixel_state()  # the camera state of the last push: the dropped last group is never walked
    assert np.array_equal(t.reshape(-1), np.array(src.last_t, np.uint32))
    assert np.array_equal(ln.reshape(-1).view(np.uint64), np.array(src.last_ln, np.float64).view(np.uint64))


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("kind,ref_time,crf", K.PPH_CASES)
def test_prophesee_case_whole_and_split(kind, ref_time, crf, device):
    case, want, src = pph(kind, ref_time, crf)
    W, H, recs = case["W"], case["H"], case["recs"]
    got, pr = run_lib(recs, W, H, ref_time, crf, device=device)
    pph_check(got, pr, want, src, len(recs))
    # cuts inside the bursts and runs, one directly after a same-t burst and one inside a clamp run
    got, pr = run_lib(recs, W, H, ref_time, crf, splits=sorted(case["cuts"].values()), device=device)
    pph_check(got, pr, want, src, len(recs))


@pytest.mark.parametrize("kind,ref_time", list(K.PPH_T0))
def test_prophesee_case_equals_the_mirror(kind, ref_time):
    import host_py as Hst
    case, want, _ = pph(kind, ref_time, None)
    W, H, recs = case["W"], case["H"], case["recs"]
    dec = P.decode(recs)
    dvs = np.zeros(len(dec), Hst.DVS_DTYPE)
    for f in ("t", "x", "y", "p"):
        dvs[f] = dec[f]
    mirror, _ = Hst.prophesee(dvs, W, H, ref_time)  # consume() and end_events; not the start-up frames
    start = len(want) - len(mirror)
    assert start == W * H and same(want[start:], mirror)


@pytest.mark.parametrize("kind,ref_time,crf", [("A", 20, 3), ("C", 1, None), ("D", 20, 3)])
def test_prophesee_bad_record_inside_a_clamp_run(kind, ref_time, crf):
    case, want, src = pph(kind, ref_time, crf)
    W, H, recs, k = case["W"], case["H"], case["recs"], case["bad_at"]
    bad = np.insert(recs, k, P.records([int(recs["t"][k])], [W], [0], [1]))  # x = W: outside the plane
    with pytest.raises(PR.BadRecord) as eo:
        PR.Prophesee(W, H, ref_time, crf).run(PR.decode_body(bad.tobytes()))
    assert eo.value.index == k
    # the whole stream in one push; then a first push that ends inside the run, the record in the second
    for first in (0, k - 5):
        pr = P.HipProphesee(W, H, ref_time, crf)
        out = [pr.start(), pr.push(recs[:first])]
        before, (t0, ln0) = pr.state(), pr.pixel_state()
        with pytest.raises(N.AdderHipError) as ei:
            pr.push(bad[first:])
        assert ei.value.code == P.E_BAD_RECORD and pr.bad_index == k and pr.state() == before
        t1, ln1 = pr.pixel_state()
        assert np.array_equal(t0, t1) and np.array_equal(ln0.view(np.uint64), ln1.view(np.uint64))
        # the refused push changed nothing: the stream without the record goes on as on a fresh context
        out += [pr.push(recs[first:]), pr.finish()]
        pph_check(np.concatenate(out), pr, want, src, len(recs))


# ---- DVS ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dvs_want(time_mode, ch, cam, ref, theta):
    case = K.dvs_case(time_mode, ch, cam, ref)
    want, bad = DR.DvsRestatement.from_meta(case["meta"], theta).run(case["ev"])
    assert bad is None
    return case, want


def wire_records(ev, ch):
    """The 9-byte (one channel) or 11-byte records of a .adder body, no EOF record."""
    if ch == 1:
        w = np.zeros(len(ev), S.WIRE9)
        w["x"], w["y"], w["d"], w["t"] = ev["x"], ev["y"], ev["d"], ev["t"]
    else:
        w = np.zeros(len(ev), S.WIRE11)
        w["x"], w["y"], w["some"], w["c"], w["d"], w["t"] = ev["x"], ev["y"], 1, ev["c"], ev["d"], ev["t"]
    return w


@pytest.mark.parametrize("time_mode,ch,cam,ref", K.DVS_CASES)
def test_dvs_case_whole_and_split(time_mode, ch, cam, ref):
    import torch
    from adder_amd import dvs
    for theta in K.DVS_THETAS:
        case, want = dvs_want(time_mode, ch, cam, ref, theta)
        meta, ev = case["meta"], case["ev"]
        w = wire_records(ev, ch)
        assert w.dtype.itemsize == (9 if ch == 1 else 11)
        dat = DR.dat_bytes(want)
        hd = dvs.HipDvs(theta=theta, **meta)  # one context, reset between the forms
        assert as_list(hd.convert(ev, dvs.OUT_EVENTS)) == want
        hd.reset()
        assert hd.convert(ev, dvs.OUT_DAT).tobytes() == dat
        hd.reset()
        assert as_list(hd.convert_wire(w.tobytes(), dvs.OUT_EVENTS)) == want and hd.consumed == len(ev)
        hd.reset()
        assert hd.convert_wire(w.tobytes(), dvs.OUT_DAT).tobytes() == dat
        # cuts between a set-up event and its window event: the window test reads ln and t from the state planes
        windows = sorted({wi for _, wi, _ in case["pairs"]})
        cuts = [0] + windows + [len(ev)]
        hd.reset()
        d = torch.from_numpy(ev.view(np.uint8).copy()).cuda()
        got = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            out = hd.convert(d[12 * a:12 * b], dvs.OUT_EVENTS)
            got += as_list(np.frombuffer(out.cpu().numpy().tobytes(), dvs.DVS_EVENT_DTYPE))
        assert got == want
        cuts = [0] + windows[::3] + [len(ev)]
        hd.reset()
        assert b"".join(hd.convert_wire(w[a:b].tobytes(), dvs.OUT_DAT).tobytes()
                        for a, b in zip(cuts[:-1], cuts[1:])) == dat
        hd.close()


@pytest.mark.parametrize("time_mode", [0, 1])
@pytest.mark.parametrize("cam", [0, K.DVS_CAM])
def test_dvs_bad_event_between_set_up_and_window(time_mode, cam):
    """An event outside the plane directly in front of a window event whose set-up event left ln = 0: the window
    event is past the limit, so it neither fires nor moves the state; the rest of the stream then gives what the
    stream without the bad event gives."""
    from adder_amd import dvs
    case, want_all = dvs_want(time_mode, 1, cam, 128, 0.01)
    meta, ev, j = case["meta"], case["ev"], case["bad_at"]
    bad = np.zeros(1, S.EVENT_DTYPE)
    bad["x"], bad["y"], bad["c"], bad["d"], bad["t"] = K.DVS_W, 0, 0xFF, 7, 100
    evb = np.insert(ev, j, bad)
    want, stop = DR.DvsRestatement.from_meta(meta).run(evb)
    assert stop == j
    hd = dvs.HipDvs(**meta)
    got = hd.convert(evb)
    assert hd.bad_index == j and as_list(got) == want
    rest = as_list(hd.convert(evb[j + 1:]))
    assert want + rest == want_all
    assert rest[0][1:] == (int(ev["x"][j]), int(ev["y"][j]), 0)  # the window event itself: the negative window arm
