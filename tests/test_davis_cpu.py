"""The DAVIS chain without a GPU (include/adder_davis.h): the Python oracle against the existing restatement, the census
of the constructed cases, and the library's shared chain code on the CPU (adder_davis_steps_host / _gaps_host /
_frame_host: the functions the kernels run) against the oracle's steps and state planes."""
import math

import numpy as np
import pytest

import adder_amd as A
import davis_cases as DC
import davis_oracle as DO
from adder_amd import davis as D

ALL = DC.CASES + DC.SEEDED


@pytest.fixture(scope="module")
def oracle_runs():
    """name -> (push results, finish events, all events, census): computed once, read only."""
    out = {}
    for case in ALL:
        census = {}
        res, fin, ev = DO.run(case["packets"], case["W"], case["H"], case["mode"], tps=case["tps"], ref_time=case["ref_time"],
                              dtm=case["dtm"], crf=case["crf"], census=census)
        out[case["name"]] = (res, fin, ev, census)
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_oracle_equals_the_mirror_tests_restatement(oracle_runs, mode):
    """Pins davis_oracle to the yardstick the mirror is already held to, on that test's seeded 38x28x7 packets."""
    from test_host_mirror import _davis_restatement
    case = DC.SEEDED[mode]
    want = _davis_restatement(case["packets"], case["W"], case["H"], mode, tps=case["tps"], ref_time=case["ref_time"],
                              dtm=case["dtm"], crf=case["crf"])
    got = oracle_runs[case["name"]][2]
    assert len(got) == len(want) > 2 * case["W"] * case["H"] and np.array_equal(got, want)


def test_constructed_cases_reach_every_arm(oracle_runs):
    total = {}
    for case in DC.CASES:
        for arm, n in oracle_runs[case["name"]][3].items():
            total[arm] = total.get(arm, 0) + n
    for lc in DC.LIST_CASES:
        DO.dvs_steps(lc["W"], lc["H"], lc["last_ts"].copy(), lc["last_ln"].copy(), lc["events"], lc["ts1"], lc["ts2"], lc["c"],
                     lc["tps"], lc["ref_time"], census=total, after2=lc["after2"])
    unreached = sorted(set(DO.ARMS) - {a for a, n in total.items() if n > 0})
    assert unreached == [], unreached
    assert set(total) <= set(DO.ARMS)


def test_tie_down_value_is_an_exact_tie():
    v, k = DC.tie_down_value()
    assert k % 2 == 0 and v * 255.0 == k + 0.5 and np.rint(v * 255.0) == k and np.rint(0.5 * 255.0) == 128


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_shared_chain_code_equals_the_oracle(oracle_runs, case):
    """Every packet phase by phase through the library's CPU forms, the planes carried from packet to packet: steps
    byte for byte, last ts exactly, last ln as bit patterns."""
    W, H, mode = case["W"], case["H"], case["mode"]
    kw = dict(tps=case["tps"], ref_time=case["ref_time"])
    ts, ln = np.zeros((H, W), np.int64), np.zeros((H, W), np.float64)
    held, end_of_last = np.zeros(0, DO.EVENT_DTYPE), None
    for pk, want in zip(case["packets"], oracle_runs[case["name"]][0]):
        start, end = 0, case["ref_time"]
        if mode != DO.FRAMED:
            start, end = int(pk["start"]), int(pk["end"])
            if mode == DO.RAW_DVS:
                end = start + 1
            s, ts, ln = D.steps_host(W, H, ts, ln, held, start, end_of_last if mode != DO.RAW_DVS else None, c=pk["c"], **kw)
            assert s.tobytes() == want["steps"]["last_after"].tobytes()
            s, ts, ln = D.steps_host(W, H, ts, ln, pk["before"], start, c=pk["c"], **kw)
            assert s.tobytes() == want["steps"]["before"].tobytes()
            s, ln = D.gaps_host(W, H, ts, ln, start, **kw)
            assert s.tobytes() == want["steps"]["gaps"].tobytes()
        img, s, ts, ln = D.frame_host(W, H, mode, pk["frame"], start, end, ts, ln)
        assert np.array_equal(img, want["image"])
        if mode != DO.FRAMED:
            assert s.tobytes() == want["steps"]["frame"].tobytes()
            held, end_of_last = pk["after"], end
        assert np.array_equal(ts, want["last_ts"])
        assert np.array_equal(_bits(ln), _bits(want["last_ln"]))


@pytest.mark.parametrize("lc", DC.LIST_CASES, ids=[c["name"] for c in DC.LIST_CASES])
def test_shared_chain_code_equals_the_oracle_with_the_second_check_in_its_other_form(lc):
    """check2_mode 2 (t < check2), which no packet path uses."""
    W, H = lc["W"], lc["H"]
    ts, ln = lc["last_ts"].copy(), lc["last_ln"].copy()
    want = DO.dvs_steps(W, H, ts, ln, lc["events"], lc["ts1"], lc["ts2"], lc["c"], lc["tps"], lc["ref_time"], after2=False)
    got = D.steps_host(W, H, lc["last_ts"], lc["last_ln"], lc["events"], lc["ts1"], lc["ts2"], check2_after=lc["after2"],
                       c=lc["c"], tps=lc["tps"], ref_time=lc["ref_time"])
    assert len(want) > 0 and got[0].tobytes() == want.tobytes()
    assert np.array_equal(got[1].reshape(-1), ts) and np.array_equal(_bits(got[2].reshape(-1)), _bits(ln))


def test_steps_host_refusals_change_nothing():
    W, H = 6, 8
    rng = np.random.default_rng(6)
    ev = DC._random_events(rng, W, H, 50, 1000, 9000)
    ts, ln = np.full((H, W), 500, np.int64), np.log1p(rng.random((H, W)))
    kw = dict(c=0.2, tps=DC.TPS, ref_time=DC.REF)

    def refused(code, **over):
        args = dict(width=W, height=H, events=ev, steps_cap=None)
        args.update(over)
        with pytest.raises(A.AdderHipError) as ei:
            D.steps_host(args["width"], args["height"], ts, ln, args["events"], 10_000, steps_cap=args["steps_cap"], **kw)
        assert ei.value.code == code
        got_ts, got_ln = ei.value.planes  # the buffers the library was given
        assert np.array_equal(got_ts, ts) and np.array_equal(_bits(got_ln), _bits(ln))
        return ei.value

    bad = ev.copy()
    bad["x"][17] = W  # one past the plane
    assert refused(D.E_BAD_EVENT, events=bad).index == 17
    bad = ev.copy()
    bad["y"][3], bad["y"][40] = H, 60000
    assert refused(D.E_BAD_EVENT, events=bad).index == 3
    e = refused(A.E_OUT_CAPACITY, steps_cap=2 * len(ev) - 1)
    assert e.needed == 2 * len(ev)
    # a height that is no multiple of 4 (the planes are 6 x 8 = 8 x 6 values)
    with pytest.raises(A.AdderHipError) as ei:
        D.steps_host(8, 6, ts.reshape(6, 8), ln.reshape(6, 8), ev[:0], 10_000, **kw)
    assert ei.value.code == A.E_BAD_PARAMS
    # and the accepted call, at the capacity the refusal named, is the plain one
    a = D.steps_host(W, H, ts, ln, ev, 10_000, steps_cap=e.needed, **kw)
    b = D.steps_host(W, H, ts, ln, ev, 10_000, **kw)
    assert len(a[0]) > 0 and a[0].tobytes() == b[0].tobytes()


def test_frame_host_refuses_nan_and_minus_one():
    W, H = 4, 4
    ts, ln = np.full((H, W), 7, np.int64), np.full((H, W), 0.25)
    for bad in (np.nan, -1.0, -3.0):
        f = np.full((H, W), 0.5)
        f[2, 1] = bad
        for mode in (D.FRAMED, D.RAW_DAVIS):
            with pytest.raises(A.AdderHipError) as ei:
                D.frame_host(W, H, mode, f, 10, 20, ts, ln)
            assert ei.value.code == A.E_BAD_PARAMS
        img, steps, ts2, ln2 = D.frame_host(W, H, D.RAW_DVS, f, 10, 11, ts, ln)  # RawDvs never reads the frame
        assert not img.any() and np.all(ts2 == 11) and np.all(ln2 == math.log1p(0.5))


def test_davis_symbols_equal_their_binding_table():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "adder_davis.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(adder_davis_\w+)\s*\(", hdr))
    assert len(names) >= 14 and names == set(D.SYMBOLS)
    L = A.load()
    for n in names:
        assert hasattr(L, n), n
    assert D.DAVIS_EVENT_DTYPE == DO.EVENT_DTYPE
    for name in ("HipDavis", "davis_to_adder", "davis_to_adder_file"):
        assert hasattr(A, name)
