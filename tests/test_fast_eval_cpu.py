"""csrc/adder_fast_logic.hpp -- the text adder_fast.hip compiles -- built by g++ (tests/cpu_sim/fast_eval_sim.cpp) against
the independent definition in tests/fast_eval_oracle.py, on every case of tests/fast_eval_cases.py: mask, score,
suppression, list order; the closed-form score against the brute force; the dense mask at threshold 30 against the
event detectors' fast9_is_feature; the confusion counts and ratios bit for bit, NaNs included.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import fast_eval_cases as K
import fast_eval_oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "adder-codec-rs_amd", "csrc")
_SRC = os.path.join(_HERE, "cpu_sim", "fast_eval_sim.cpp")
_MAIN = os.path.join(_HERE, "cpu_sim", "fast_eval_main.cpp")
_LIB = os.path.join(_HERE, "cpu_sim", "libadder_fast_eval_sim.so")
_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-I", _CSRC]


@pytest.fixture(scope="module")
def sim():
    deps = [_SRC] + [os.path.join(_CSRC, n) for n in ("adder_fast_logic.hpp", "adder_pixel.hpp")]
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", *_FLAGS, "-fPIC", "-shared", _SRC, "-o", _LIB])
    L = C.CDLL(_LIB)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.fes_detect.restype = u64
    L.fes_detect.argtypes = [vp, u32, u32, u32, C.c_int, C.c_int, vp, vp, vp]
    L.fes_raw_score.argtypes = [vp, u32, u32, u32, vp]
    L.fes_fast9_plane.argtypes = [vp, u32, u32, u32, vp]
    L.fes_confusion.argtypes = [vp, vp, u64, vp, vp]
    return L


def sim_detect(L, frame, threshold, nonmax):
    frame = np.ascontiguousarray(frame, np.uint8)
    h, w = frame.shape[:2]
    ch = 1 if frame.ndim == 2 else frame.shape[2]
    mask, score, xy = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), np.zeros(h * w, np.uint32)
    n = L.fes_detect(frame.ctypes.data, w, h, ch, threshold, int(nonmax), mask.ctypes.data, score.ctypes.data,
                     xy.ctypes.data)
    assert n <= h * w, "the list and the mask disagree"
    return mask, score, xy[:n]


_ORACLE = {}


def oracle(name, threshold, nonmax):
    """Computed once per (case, threshold, suppression), shared by the tests below."""
    key = (name, threshold, nonmax)
    if key not in _ORACLE:
        _ORACLE[key] = [O.detect(f, threshold, nonmax) for f in K.CASES[name].frames]
    return _ORACLE[key]


def _points():
    return [(n, t, nm) for n, c in K.CASES.items() for t in c.thresholds for nm in (False, True)]


def test_census():
    """Every case still shows what it is there for."""
    assert set(K.CENSUS) == set(K.CASES) - {"noise_and_squares"}
    for name, want in K.CENSUS.items():
        plain = oracle(name, 30, False)
        nonmax = oracle(name, 30, True)
        n_plain = sum(len(r[2]) for r in plain)
        n_nonmax = sum(len(r[2]) for r in nonmax)
        # a tie: two horizontally adjacent corners of equal score
        ties = sum(int(((r[1][:, 1:] == r[1][:, :-1]) & (r[1][:, 1:] > 0)).sum()) for r in plain)
        top = max(int(r[1].max()) for r in plain)
        for k, v in want.items():
            got = {"plain": n_plain, "nonmax": n_nonmax, "ties": ties, "max_score": top}[k.replace("_min", "")]
            assert (got >= v) if k.endswith("_min") else (got == v), (name, k, got, v)
    m = oracle("edge_corners", 30, False)[0][0]
    h, w = m.shape
    assert m[3, 3] and m[3, w - 4] and m[h - 4, 3] and m[h - 4, w - 4] and not m[8, 2] and not m[h - 3, 11]


@pytest.mark.parametrize("name,threshold,nonmax", _points())
def test_logic_header_equals_the_oracle(sim, name, threshold, nonmax):
    for frame, (mask, score, xy) in zip(K.CASES[name].frames, oracle(name, threshold, nonmax)):
        got_mask, got_score, got_xy = sim_detect(sim, frame, threshold, nonmax)
        assert np.array_equal(got_score, score)
        assert np.array_equal(got_mask, mask)
        assert np.array_equal(got_xy, xy)  # raster order
        if not nonmax:
            assert np.array_equal(mask != 0, O.dense_fast(frame, threshold))  # the walk itself, not via the score


def test_three_channels_read_channel_zero(sim):
    plane = K.noise_and_squares(45, 29, 11)[0]
    decoy = K.noise(45, 29, 12, n=2)
    frame = np.stack([plane, decoy[0], decoy[1]], axis=-1)
    for nonmax in (False, True):
        want = O.detect(plane, 30, nonmax)
        got = sim_detect(sim, frame, 30, nonmax)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert all(np.array_equal(g, w) for g, w in zip(O.detect(frame, 30, nonmax), want))


def test_closed_form_score_equals_brute_force(sim):
    """max over the arcs of the arc's minimum, less one, is the largest threshold the literal walk accepts -- at every
    candidate of every case, also those below the threshold in use (negative: a corner at no threshold, the brute
    force's -1)."""
    for name, case in K.CASES.items():
        for frame in case.frames:
            h, w = frame.shape
            raw = np.zeros((h, w), np.int32)
            sim.fes_raw_score(np.ascontiguousarray(frame).ctypes.data, w, h, 1, raw.ctypes.data)
            ys, xs, c, ring = O._centres_and_rings(frame)
            best = np.full(len(ys), -1, np.int32)
            for t in range(255):
                best[O.walk(c, ring, t)] = t
            assert np.array_equal(np.maximum(raw[ys, xs], -1), best), name
            assert raw.max(initial=0) <= 254 and not O.walk(c, ring, 255).any()


def test_threshold_30_is_the_event_detectors_test(sim):
    for name, case in K.CASES.items():
        for frame, (mask, _, _) in zip(case.frames, oracle(name, 30, False)):
            h, w = frame.shape
            got = np.zeros((h, w), np.uint8)
            sim.fes_fast9_plane(np.ascontiguousarray(frame).ctypes.data, w, h, 1, got.ctypes.data)
            assert np.array_equal(got, mask), name


def _same_bits(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b) or (a != a and b != b)


def test_confusion_bit_for_bit(sim):
    seen_nan = set()
    for name in ("constant", "noise", "squares", "equal_pair", "one_candidate_7x7", "no_candidates_6x9"):
        for nonmax in (False, True):
            truth = oracle(name, 30, nonmax)[0][0]
            for pname, pred in K.predictions(truth).items():
                want = O.precision_recall_accuracy(truth, pred)
                counts, ratios = np.zeros(4, np.uint64), np.zeros(3, np.float64)
                sim.fes_confusion(np.ascontiguousarray(truth).ctypes.data, pred.ctypes.data, truth.size,
                                  counts.ctypes.data, ratios.ctypes.data)
                assert [int(x) for x in counts] == [want[k] for k in ("tp", "fp", "tn", "fn")], (name, pname)
                for got, k in zip(ratios, ("precision", "recall", "accuracy")):
                    assert _same_bits(float(got), want[k]), (name, pname, k, got, want[k])
                    if want[k] != want[k]:
                        seen_nan.add(k)
                if name == "constant" and pname == "empty":
                    assert want["precision"] != want["precision"] and want["recall"] != want["recall"]
                    assert want["accuracy"] == 1.0
    assert seen_nan == {"precision", "recall"}


def test_stand_alone_program(tmp_path):
    """tests/cpu_sim/fast_eval_main.cpp (the program sanitizer builds of the header run) over the case list."""
    exe, casefile = str(tmp_path / "fast_eval_main"), str(tmp_path / "cases.bin")
    subprocess.check_call(["g++", *_FLAGS, _MAIN, "-o", exe])
    want = []
    with open(casefile, "wb") as fh:
        for name, case in K.CASES.items():
            for nonmax in (False, True):
                for frame, (mask, score, xy) in zip(case.frames, oracle(name, 30, nonmax)):
                    h, w = frame.shape
                    fh.write(struct.pack("<5I", w, h, 1, 30, int(nonmax)) + frame.tobytes())
                    pred = (np.arange(h * w) % 3 == 0).reshape(h, w)
                    c = O.precision_recall_accuracy(mask, pred)
                    csum = 0
                    for v in xy:
                        csum = (csum * 1000003 + int(v)) % (1 << 64)
                    want.append((len(xy), int(score.sum(dtype=np.int64)), csum, c["tp"], c["fp"], c["tn"], c["fn"]))
    out = subprocess.run([exe, casefile], check=True, capture_output=True, text=True).stdout
    got = [tuple(int(x) for x in line.split()) for line in out.splitlines()]
    assert got == want
