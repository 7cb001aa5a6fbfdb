"""The constructed chain cases (tests/chain_arm_cases.py) without a GPU: each reaches the arms it is built for, by the
census of the oracles (tests/chain_arms.py); the random inputs of the older GPU tests do not; and the oracles equal
the library's host exp and log1p on them -- the routines the kernels evaluate -- so that a mismatch on the device
points at a kernel."""
import math

import numpy as np
import pytest

import chain_arm_cases as K
import chain_arms as A
import dvs_oracle as DR
import prophesee_oracle as PR
from adder_amd import prophesee as P


# ---- Prophesee ----------------------------------------------------------------------------------------------------

def _closing_indices(recs):
    """consume()'s reading loop: the index of every record that closes a group."""
    start, rt, out = 2, 2, []
    for i, t in enumerate(recs["t"].tolist()):
        rt = max(rt, t)
        if t > ((start + PR.VIEW_INTERVAL) & PR.M32):
            out.append(i)
            start = rt
    return out


@pytest.mark.parametrize("kind,ref_time,crf", K.PPH_CASES)
def test_prophesee_case_reaches_its_arms(kind, ref_time, crf):
    case = K.prophesee_case(kind, ref_time)
    recs = case["recs"]
    assert len(recs) <= 4000 and (case["W"], case["H"]) == (16, 12)
    cen, src, ev = A.prophesee_census(recs, case["W"], case["H"], ref_time, crf)
    assert cen.missing(K.pph_arms(kind, ref_time)) == [], dict(cen.count)
    if kind == "A":
        assert not any(cen.count[a] for a in ("t_over_2p24", "t_over_2p31", "gap_time_wrap", "end_span_wrap"))
    # the census changes nothing
    plain = PR.Prophesee(case["W"], case["H"], ref_time, crf)
    assert plain.run(PR.decode_body(recs.tobytes())).tobytes() == ev.tobytes()
    assert plain.last_t == src.last_t and plain.last_ln == src.last_ln
    # four runs and two bursts lie on both sides of a group boundary: the state crosses a launch in mid-run
    closing = _closing_indices(recs)
    assert len(closing) >= 7
    spanned = {name for (name, _), (a, b) in case["runs"].items() if any(a <= c < b for c in closing)}
    assert spanned >= {"H1", "L1", "H2", "L2", "G1", "K1"}, spanned
    # every constructed record is walked: none lies in the dropped last group
    assert max(b for _, b in case["runs"].values()) < closing[-1]
    # the cuts of the GPU test fall where they are meant to
    cuts, runs = case["cuts"], case["runs"]
    a, b = runs[("H1", K.pph_boundary(0) - 20)]
    assert a < cuts["inside_clamp_run"] <= b
    a, b = runs[("G2", 7000)]
    assert cuts["after_same_t_burst"] == b + 1
    a, b = runs[("K2", 11000)]
    assert a < cuts["inside_burst"] <= b
    a, b = runs[("H2", K.pph_boundary(4) - 40)]
    assert a < case["bad_at"] < b


def test_the_random_recordings_lack_the_gap_clamp():
    from test_gpu_prophesee import recording
    cen, _, _ = A.prophesee_census(recording(101, 46, 30, 6000), 46, 30, 1, None)
    assert cen.count["gap"] > 1000
    for arm in ("gap_clamp_hi", "gap_clamp_lo", "step_clamp_lo", "gap_time_wrap", "t_over_2p24", "end_span_wrap"):
        assert cen.count[arm] == 0, arm


@pytest.mark.parametrize("kind,ref_time", list(K.PPH_T0))
def test_prophesee_oracle_equals_the_host_exp(kind, ref_time, monkeypatch):
    """The restatement over the library's host exp (the routine the walk kernel evaluates) gives the same events
    and the same camera state.  (The C++ mirror drives the device's integrator: tests/test_gpu_chain_arms.py
    compares with it.)"""
    import types
    case = K.prophesee_case(kind, ref_time)
    body = PR.decode_body(case["recs"].tobytes())
    want = PR.Prophesee(case["W"], case["H"], ref_time)
    ev = want.run(body)
    monkeypatch.setattr(PR, "math", types.SimpleNamespace(exp=P.exp, log1p=math.log1p))
    got = PR.Prophesee(case["W"], case["H"], ref_time)
    assert got.run(body).tobytes() == ev.tobytes()
    assert got.last_t == want.last_t and got.last_ln == want.last_ln


# ---- DVS ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("time_mode,ch,cam,ref", K.DVS_CASES)
def test_dvs_case_reaches_its_arms(time_mode, ch, cam, ref):
    case = K.dvs_case(time_mode, ch, cam, ref)
    meta, ev = case["meta"], case["ev"]
    assert len(ev) <= 4000 and (meta["width"], meta["height"]) == (6, 5)
    for theta in K.DVS_THETAS:
        cen, out, bad = A.dvs_census(meta, ev, theta)
        assert bad is None
        assert cen.missing(K.dvs_arms(time_mode, cam, ref, theta)) == [], (theta, dict(cen.count))
        assert DR.DvsRestatement.from_meta(meta, theta).run(ev) == (out, None)  # the census changes nothing
    # the constructed units sort between filler units, and each window event follows its set-up event
    units = {(int(e["y"]), int(e["x"]), 0 if e["c"] == 0xFF else int(e["c"])) for e in ev}
    mine = {(y, x, 0 if ch == 1 else 1) for x, y in K.DVS_UNITS}
    assert mine <= units and min(units) < min(mine) and max(mine) < max(units)
    assert all(s < w for s, w, _ in case["pairs"]) and len(case["pairs"]) >= 24


@pytest.mark.parametrize("time_mode", [0, 1])
@pytest.mark.parametrize("cam", [0, K.DVS_CAM])
def test_dvs_same_time_directly_after_the_first_event(time_mode, cam):
    """ref 128: the first event leaves ln in (0.6, win_hi] (units 0, 1) or [win_lo, 0.3) (units 2, 3); a window event
    at the same time follows.  A framed camera rounds the time up unless the first time is a multiple of ref (units
    0, 2): on units 1, 3 the same-time arm must not be taken, and the half-threshold test gives the other polarity."""
    case = K.dvs_case(time_mode, 1, cam, 128)
    assert len(case["first_pairs"]) == 4
    for ui, (s, w, _) in enumerate(case["first_pairs"]):
        x, y = K.DVS_UNITS[ui]
        cen = A.Census()
        r = DR.DvsRestatement.from_meta(case["meta"])
        r.census = cen
        out, _ = r.run(case["ev"][: w + 1], units={(y, x, 0)})
        taken = cam == K.DVS_CAM or ui in (0, 2)
        arm = ("win_same_hi" if ui < 2 else "win_same_lo") if taken else ("down" if ui < 2 else "up")
        assert cen.count[arm] == 1 and sum(cen.count[a] for a in ("win_same_hi", "win_same_lo", "up", "down")) == 1
        first_t = int(case["ev"][s]["t"])
        assert out == [(first_t + 1, x, y, 1 if arm in ("win_same_hi", "up") else 0)]


def test_the_fuzz_streams_lack_three_window_arms():
    from test_gpu_dvs import random_stream
    ch, time_mode, cam, ref = 1, 0, 0, 255
    rng = np.random.default_rng(ch * 1000 + time_mode * 100 + cam * 10 + ref)
    ev = random_stream(rng, 6000, 6, 5, ch, big_t=True)
    meta = dict(width=6, height=5, channels=ch, time_mode=time_mode, ref_interval=ref, source_camera=cam)
    for theta in (0.01, 0.0, 0.3):
        cen, _, _ = A.dvs_census(meta, ev, theta)
        assert cen.count["up"] > 100
        for arm in ("win_lo", "win_same_hi", "win_same_lo"):
            assert cen.count[arm] == 0, (theta, arm)


@pytest.mark.parametrize("time_mode,ch,cam,ref", K.DVS_CASES)
def test_dvs_oracle_equals_the_host_log1p(time_mode, ch, cam, ref, monkeypatch):
    """The restatement over the library's host log1p (the routine the kernels evaluate) gives the same output, and
    every intensity of the case is the same double."""
    from adder_amd import dvs
    case = K.dvs_case(time_mode, ch, cam, ref)
    want = DR.DvsRestatement.from_meta(case["meta"]).run(case["ev"])
    args = []

    def host_ln(d, t, r):
        if d == DR.D_ZERO_INTEGRATION:
            return 0.0
        p = float(1 << d)
        x = (p * float(r)) / 255.0 if t == 0 else ((p / float(t)) * float(r)) / 255.0
        args.append(x)
        return dvs.log1p(x)
    monkeypatch.setattr(DR, "intensity_ln", host_ln)
    assert DR.DvsRestatement.from_meta(case["meta"]).run(case["ev"]) == want
    x = np.array(args)
    assert len(x) > 2000
    assert np.array_equal(dvs.log1p(x).view(np.uint64), np.array([math.log1p(v) for v in args]).view(np.uint64))
