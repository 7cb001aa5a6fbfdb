"""ADDER -> DVS (include/adder_dvs.h) without a GPU: hand-derived known answers of the restatement
(tests/dvs_oracle.py) for every rule of adder-to-dvs/src/main.rs, the output formats, the library's host log1p
against the platform libm bit for bit, its header parser on every golden, its symbol table and the C example."""
import gzip
import math
import os
import re
import subprocess

import numpy as np
import pytest

import adder_stream_np as S
import dvs_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLDENS = ["adder_info_test_sample.adder", "bunny_v2_dt.adder", "bunny_v2_t.adder", "nyc_v1_1px.adder",
           "nyc_source_v2_2_1px.adder", "sample_3_ordered.adder", "sample_3_unordered.adder", "virat_small_gray.adder",
           "lake_scaled_hd_out.adder.gz"]
DVS_CAM = 6  # SourceCamera::Dvs: not framed
NONE = 0xFF


def golden_bytes(name):
    path = os.path.join(GOLDEN, name)
    return gzip.open(path).read() if name.endswith(".gz") else open(path, "rb").read()


def run(events, w=4, h=1, ch=1, time_mode=0, ref=255, cam=DVS_CAM, theta=0.01):
    r = R.DvsRestatement(w, h, ch, time_mode, ref, cam, theta)
    out, bad = r.run([(x, 0, NONE, d, t) if ch == 1 else (x, 0, c, d, t) for x, c, d, t in events])
    return out, bad, r


def I(d, t, ref):
    return R.intensity_ln(d, t, ref)


# ---- known answers ----------------------------------------------------------------------------------------------

def test_first_event_emits_nothing_and_sets_the_state():
    out, bad, r = run([(0, 0, 7, 100)])
    assert out == [] and bad is None
    assert r.px[(0, 0, 0)] == [7, math.log1p((128.0 / 100.0) * 255.0 / 255.0), 100]


def test_d_zero_integration_and_t_zero_branches():
    assert I(128, 77, 255) == 0.0
    assert I(5, 0, 255) == math.log1p((32.0 * 255.0) / 255.0)
    assert I(5, 3, 5000) == math.log1p(((32.0 / 3.0) * 5000.0) / 255.0)


def test_delta_t_accumulates_and_a_framed_camera_rounds_up():
    ev = [(0, 0, 7, 100), (0, 0, 7, 100), (0, 0, 8, 100)]
    out, _, r = run(ev, cam=0)  # FramedU8: 100 -> 200 rounds to 255 -> 355 rounds to 510
    assert out == [(256, 0, 0, 1)] and r.px[(0, 0, 0)][2] == 510
    out, _, r = run(ev, cam=DVS_CAM)
    assert out == [(201, 0, 0, 1)] and r.px[(0, 0, 0)][2] == 300


def test_absolute_t_saturating_sub_with_a_truncated_old_t():
    ev = [(0, 0, 7, 0xFFFFFFF0), (0, 0, 7, 0xFFFFFFFF), (0, 0, 7, 3000), (0, 0, 7, 1000)]
    out, _, r = run(ev, time_mode=1, ref=5000, cam=0)
    # 2: dt = 15, px.t = 0xFFFFFFFF rounded up to 4294970000 (> 2^32): positive at the first event's raw t + 1
    # 3: old_t as u32 = 2704, dt = 296: negative at 4294970001; px.t = 5000
    # 4: 1000 - 5000 saturates to 0 (the t == 0 branch): positive
    assert out == [(0xFFFFFFF1, 0, 0, 1), (4294970001, 0, 0, 0), (5001, 0, 0, 1)]
    assert r.px[(0, 0, 0)][1] == I(7, 0, 5000)


def test_d_empty_moves_the_time_and_fires_nothing():
    out, _, r = run([(0, 0, 7, 100), (0, 0, 255, 1000), (0, 0, 8, 100)])
    assert out == [(1101, 0, 0, 1)]


def test_window_branches():
    # ref 128: a t == 0 event with d == 0 has ln_1p(128 / 255) = 0.40678, inside (0.406, 0.407)
    assert 0.406 < I(0, 0, 128) < 0.407
    # positive window: the old intensity above ln_1p(1) - theta (0.6931 > 0.6831) -- theta alone would say negative
    out, _, _ = run([(0, 0, 1, 1), (0, 0, 0, 0)], ref=128)
    assert I(1, 1, 128) > math.log1p(1.0) - 0.01 and out == [(2, 0, 0, 1)]
    # ... or above 0.6 with px.t == old_t (a zero delta)
    assert 0.6 < I(4, 9, 128) < math.log1p(1.0) - 0.01
    out, _, _ = run([(0, 0, 4, 9), (0, 0, 0, 0)], ref=128)
    assert out == [(10, 0, 0, 1)]
    out, _, _ = run([(0, 0, 4, 9), (0, 0, 0, 1), (0, 0, 0, 0)], ref=128)  # t moved: the theta test, negative
    assert out[0] == (10, 0, 0, 0)
    # negative window: old below ln_1p(0) + theta (d == 128 gives 0.0) -- theta alone would say positive
    out, _, _ = run([(0, 0, 128, 5), (0, 0, 0, 0)], ref=128)
    assert out == [(6, 0, 0, 0)]
    # ... or below 0.3 with px.t == old_t
    assert 0.01 < I(0, 2, 128) < 0.3
    out, _, _ = run([(0, 0, 0, 2), (0, 0, 0, 0)], ref=128)
    assert out == [(3, 0, 0, 0)]


def test_theta_half_branches_and_theta_zero():
    out, _, r = run([(0, 0, 7, 100), (0, 0, 8, 100)])
    assert out == [(101, 0, 0, 1)] and r.px[(0, 0, 0)][1] == I(8, 100, 255)
    out, _, _ = run([(0, 0, 8, 100), (0, 0, 7, 100)])
    assert out == [(101, 0, 0, 0)]
    # a change of 0.0028 (< theta / 2 = 0.005): nothing at theta 0.01, negative at theta 0; no change: nothing
    ev = [(0, 0, 7, 100), (0, 0, 8, 201), (0, 0, 8, 201)]
    assert 0 < I(7, 100, 255) - I(8, 201, 255) < 0.005
    assert run(ev)[0] == []
    assert run(ev, theta=0.0)[0] == [(101, 0, 0, 0)]


def test_units_are_separate_and_bad_events_stop_the_run():
    out, bad, _ = run([(0, 0, 7, 100), (1, 0, 7, 100), (1, 0, 8, 100), (0, 0, 8, 100)])
    assert out == [(101, 1, 0, 1), (101, 0, 0, 1)] and bad is None
    assert run([(0, 0, 7, 1), (0, 0, 8, 1), (0, 0, 200, 1), (0, 0, 9, 1)])[:2] == ([(2, 0, 0, 1)], 2)
    assert run([(0, 0, 255, 1)])[:2] == ([], 0)  # a unit's first event with d > 128
    assert run([(0, 0, 7, 1), (9, 0, 7, 1)])[:2] == ([], 1)  # outside the plane


def test_binary_packing_and_text():
    assert R.dat_bytes([(5, 20000, 3, 1)]) == (5).to_bytes(4, "little") + \
        ((1 << 28) | (3 << 14) | 20000).to_bytes(4, "little")  # x is not masked
    assert R.dat_bytes([((1 << 32) + 7, 1, 2, 0)])[:4] == (7).to_bytes(4, "little")
    assert R.text_bytes([((1 << 32) + 7, 1, 2, 0)]) == b"4294967303 1 2 0\n"


def test_header_bytes_both_modes():
    from adder_amd import dvs
    want = b"% Height 50\n% Width 200\n% Version 2\n% Date 2024-05-06 07:08:09\n% end\n"
    assert dvs.header_bytes(200, 50, "2024-05-06 07:08:09", binary=False) == want
    assert dvs.header_bytes(200, 50, "2024-05-06 07:08:09", binary=True) == want + b"\x00\x08"
    assert R.header_bytes(200, 50, "2024-05-06 07:08:09", True) == want + b"\x00\x08"


def test_text_formatter():
    from adder_amd import dvs
    ev = np.zeros(3, dvs.DVS_EVENT_DTYPE)
    ev["t"], ev["x"], ev["y"], ev["p"] = [1, (1 << 40) + 3, 0], [0, 65535, 2], [9, 1, 0], [1, 0, 1]
    out = [(int(e["t"]), int(e["x"]), int(e["y"]), int(e["p"])) for e in ev]
    assert dvs.format_text(ev) == R.text_bytes(out)


# ---- the library's host log1p ------------------------------------------------------------------------------------

def _sweep_args():
    """every d in 0..=127 with t in {0, 1..65536, 2^k +- 1}, and 10^6 random (d, u32 t), for ref 255 and 5000"""
    rng = np.random.default_rng(5)
    ts = np.unique(np.concatenate([np.arange(0, 65537), (1 << np.arange(1, 33, dtype=np.uint64)) - 1,
                                   (1 << np.arange(1, 32, dtype=np.uint64)) + 1]).astype(np.uint64))
    d = np.concatenate([np.repeat(np.arange(128), ts.size), rng.integers(0, 128, 1_000_000)])
    t = np.concatenate([np.tile(ts, 128), rng.integers(0, 1 << 32, 1_000_000, dtype=np.uint64)])
    xs = []
    for ref in (255.0, 5000.0):
        p = np.ldexp(1.0, d)
        xs.append(np.where(t == 0, (p * ref) / 255.0, ((p / np.maximum(t, 1).astype(np.float64)) * ref) / 255.0))
    return np.concatenate(xs)


def _golden_args():
    xs = []
    for name in GOLDENS:
        meta, ev, _ = S.read_adder(golden_bytes(name))
        ok = ev["d"] < 128
        d, t = ev["d"][ok].astype(np.int64), ev["t"][ok].astype(np.uint64)
        p = np.ldexp(1.0, d)
        ref = float(meta["ref_interval"])
        xs.append(np.where(t == 0, (p * ref) / 255.0, ((p / np.maximum(t, 1).astype(np.float64)) * ref) / 255.0))
    return np.concatenate(xs)


@pytest.mark.parametrize("which", ["sweep", "goldens"])
def test_host_log1p_equals_libm_bit_for_bit(which):
    from adder_amd import dvs
    x = _sweep_args() if which == "sweep" else _golden_args()
    got = dvs.log1p(x)
    want = np.array([math.log1p(v) for v in x.tolist()])
    diff = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert diff.size == 0, (diff.size, x[diff[:5]])
    for v in (0.0, 1.0, 1e-300, 2.0 ** -30, 2.0 ** -60, 0.41, 0.4142, 1e300, float("inf"), -0.25, -0.5):
        assert math.copysign(1, dvs.log1p(v)) == math.copysign(1, math.log1p(v)) and dvs.log1p(v) == math.log1p(v)


# ---- header parser, symbols, example ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", GOLDENS)
def test_header_parser_on_every_golden(name):
    from adder_amd import dvs
    buf = golden_bytes(name)
    meta, hb, eb = dvs.parse_header(buf)
    want = S.parse_header(buf)
    assert hb == want["header_size"] and eb == want["event_size"]
    for k in ("width", "height", "channels", "time_mode", "ref_interval", "source_camera"):
        assert meta[k] == want[k], k


def test_header_parser_refuses_what_is_not_a_header():
    from adder_amd import dvs, AdderHipError
    buf = bytearray(golden_bytes("bunny_v2_dt.adder")[:64])
    for bad in (b"", bytes(buf[:20]), b"xdder" + bytes(buf[5:]), bytes(buf[:5]) + b"\x09" + bytes(buf[6:])):
        with pytest.raises(AdderHipError):
            dvs.parse_header(bad)


def test_dvs_symbols_equal_their_binding_table():
    import ctypes
    import adder_amd
    from adder_amd import dvs
    hdr = open(os.path.join(ROOT, "include", "adder_dvs.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(adder_dvs_\w+)\s*\(", hdr))
    assert len(names) >= 14 and names == set(dvs.SYMBOLS)
    adder_amd.load()
    L = ctypes.CDLL(adder_amd.LIB_PATH)
    for n in names:
        assert hasattr(L, n), n


def build_example(tmp_path):
    import adder_amd
    adder_amd.load()
    lib = os.path.join(ROOT, "adder-codec-rs_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "adder_to_dvs")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "examples", "adder_to_dvs.c"), "-L", lib, "-ladder_hip",
                           "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + lib,
                           "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe])
    return exe


def test_dvs_example_compiles_with_warnings_as_errors(tmp_path):
    assert os.path.exists(build_example(tmp_path))
