"""The latest-event player (include/adder_player.h) without a GPU: hand-derived known answers of the restatement
(tests/player_oracle.py) for every rule of adder_video_player.rs, the library's display schedule (a prefix minimum)
against the serial loop, its header parser on every golden, the refused cameras and parameters, its symbol table and
the C example."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import adder_stream_np as S
import player_oracle as R
from test_dvs_cpu import GOLDENS, golden_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFF
DVS_CAM = 6


def player(time_mode=0, ref=255, tps=15300, cam=0, fps=60.0, w=4, h=1, ch=1):
    """tps 15300 at 60 fps: FL = 255"""
    return R.PlayerRestatement(w, h, ch, time_mode, ref, tps, cam, fps)


def ev(x, d, t, c=NONE):
    return (x, 0, c, d, t)


# ---- known answers, rule by rule --------------------------------------------------------------------------------

def test_first_event_value():
    for mode in (0, 1):  # the first event's time is t in both modes (last_ts starts at 0)
        p = player(mode)
        p.run([ev(0, 7, 255)])
        v = p.display[0, 0, 0]
        assert v == ((128.0 / 255.0) * 255.0) / 255.0  # a division, a multiplication, a division
        assert abs(v - 128.0 / 255.0) <= 2.0 ** -53 and p.display[0, 1, 0] == 0.0


def test_t_zero_is_treated_as_one_and_d_128_is_zero():
    p = player(0, ref=5000)
    p.run([ev(0, 5, 0), ev(1, 128, 77), ev(2, 5, 3)])
    assert p.display[0, 0, 0] == (32.0 * 5000.0) / 255.0
    assert p.display[0, 1, 0] == 0.0
    assert p.display[0, 2, 0] == ((32.0 / 3.0) * 5000.0) / 255.0
    assert R.event_to_intensity(128, 0) == 0.0 and R.event_to_intensity(0, 0) == 1.0
    assert R.event_to_intensity(127, 1) == 2.0 ** 127


def test_the_divisor_follows_the_source_camera():
    for cam, m in ((0, 255.0), (1, 65535.0), (2, 4294967295.0), (3, 18446744073709551616.0), (6, 255.0), (7, 255.0)):
        p = player(0, cam=cam)
        p.run([ev(0, 9, 10)])
        assert p.display[0, 0, 0] == ((512.0 / 10.0) * 255.0) / m
    for cam in (4, 5, 8, 9):
        with pytest.raises(KeyError):
            player(0, cam=cam)


def test_d_above_128_changes_nothing_but_its_iteration_checks():
    # FL 255.  The first event puts current_t at 1020 = 4 FL: frames at the checks of the next records, whatever their d
    p = player(0)
    frames, bad = p.run([ev(0, 7, 1020), ev(1, 129, 999999), ev(9, 255, 5), ev(1, 200, 1)])
    assert bad is None  # d > 128 never indexes the plane: x = 9 is outside it
    assert len(frames) == 3 and p.frame_count == 4 and p.current_t == 1020
    for f in frames:
        assert f[0, 0, 0] == ((128.0 / 1020.0) * 255.0) / 255.0 and f[0, 1, 0] == 0.0
    assert p.last_ts[0, 1, 0] == 0 and p.display[0, 1, 0] == 0.0


def test_absolute_t_delta_and_round_up():
    p = player(1)
    p.run([ev(0, 7, 100), ev(0, 7, 300)])
    # last_ts: 100 -> 255; the second event's time is 300 - 255 = 45; last_ts 300 -> 510; current_t is the raw t
    assert p.display[0, 0, 0] == ((128.0 / 45.0) * 255.0) / 255.0
    assert p.last_ts[0, 0, 0] == 510 and p.current_t == 300
    p = player(1)
    p.run([ev(0, 7, 510), ev(1, 7, 20)])  # a multiple stays; current_t never goes back
    assert p.last_ts[0, 0, 0] == 510 and p.last_ts[0, 1, 0] == 255 and p.current_t == 510


def test_other_modes_accumulate_and_round_up():
    for mode in (0, 2):  # DeltaT and Mixed: everything that is not AbsoluteT
        p = player(mode)
        p.run([ev(0, 7, 100), ev(0, 8, 100)])
        # 100 -> 255; 255 + 100 = 355 -> 510; the event's time stays 100; current_t is the rounded last_ts
        assert p.last_ts[0, 0, 0] == 510 and p.current_t == 510
        assert p.display[0, 0, 0] == ((256.0 / 100.0) * 255.0) / 255.0


def test_round_up_applies_to_a_non_framed_camera_too():
    for mode, want in ((0, 510), (1, 510)):
        p = player(mode, cam=DVS_CAM)
        p.run([ev(0, 7, 100), ev(0, 7, 300 if mode else 100)])
        assert p.last_ts[0, 0, 0] == want


def test_u32_wrap_in_both_modes():
    # AbsoluteT, ref 1000: 0xFFFFFFF0 = 4294967280 rounds up to 4294968000 = 2^32 + 704
    p = player(1, ref=1000)
    p.run([ev(0, 7, 0xFFFFFFF0)])
    assert p.last_ts[0, 0, 0] == 704 and p.current_t == 0xFFFFFFF0
    p.run([ev(0, 7, 1000)])
    assert p.display[0, 0, 0] == ((128.0 / 296.0) * 1000.0) / 255.0  # 1000 - 704
    p.run([ev(0, 7, 100)])  # last_ts is 1000: 100 - 1000 wraps to 2^32 - 900
    assert p.display[0, 0, 0] == ((128.0 / 4294966396.0) * 1000.0) / 255.0
    assert p.current_t == 0xFFFFFFF0
    # accumulating: the round-up wraps (4294967040 -> 4294968000 = 2^32 + 704) ...
    p = player(0, ref=1000)
    p.run([ev(0, 7, 0xFFFFFF00)])
    assert p.last_ts[0, 0, 0] == 704 and p.current_t == 704
    # ... and so does the sum: 4294967000 + 500 = 2^32 + 204, rounded up to 1000
    p = player(0, ref=1000)
    p.run([ev(0, 7, 4294967000), ev(0, 7, 500)])
    assert p.last_ts[0, 0, 0] == 1000 and p.current_t == 4294967000
    assert p.display[0, 0, 0] == ((128.0 / 500.0) * 1000.0) / 255.0


def test_the_display_comparison_is_strict():
    p = player(0)
    frames, _ = p.run([ev(0, 7, 255), ev(1, 7, 1)], end=True)  # current_t == 1 * FL at both later checks
    assert frames == [] and p.current_t == 255 and p.frame_count == 1
    p = player(1)
    frames, _ = p.run([ev(0, 7, 256), ev(1, 7, 1)], end=True)  # 256 > 255: one frame; then 256 > 510 is false
    assert len(frames) == 1 and p.frame_count == 2
    assert frames[0][0, 1, 0] == 0.0  # shown before the second event was applied


def test_the_last_check_before_eof():
    events = [ev(0, 7, 10), ev(1, 7, 2000)]
    p = player(1)
    frames, _ = p.run(events, end=True)  # the last event crosses a boundary: only the EOF iteration's check shows it
    assert len(frames) == 1 and frames[0][0, 1, 0] == ((128.0 / 2000.0) * 255.0) / 255.0
    p = player(1)
    frames, _ = p.run(events)
    assert frames == []
    assert len(p.finish()) == 1 and p.frame_count == 2
    assert R.PlayerRestatement(4, 1, 1, 1, 255, 15300, 0).run([], end=True) == ([], None)  # N = 0: one check, no frame


def test_at_most_one_frame_per_iteration_and_fl_zero():
    p = player(1)
    frames, _ = p.run([ev(0, 7, 255 * 10 + 1)] + [ev(1, 200, 0)] * 3, end=True)
    assert len(frames) == 4  # ten boundaries passed, four checks followed
    p = player(1, tps=30, fps=60.0)  # FL = 0: every check with current_t > 0 shows a frame
    assert p.fl == 0
    frames, _ = p.run([ev(0, 7, 0), ev(0, 7, 1), ev(1, 7, 1), ev(1, 7, 1)], end=True)
    assert len(frames) == 3


def test_an_event_outside_the_plane_ends_the_batch_before_it():
    p = player(1)
    frames, bad = p.run([ev(0, 7, 2000), ev(4, 7, 1), ev(1, 7, 1)])
    assert bad == 1 and frames == [] and p.frame_count == 1  # no check at the bad index
    p = player(1, ch=3)
    assert p.run([ev(0, 7, 1, c=3)])[1] == 0
    assert p.run([(0, 1, 0, 7, 1)])[1] == 0


def test_frame_length_truncates_and_saturates():
    from adder_amd import player as P
    for tps, fps in ((15300, 60.0), (7650, 60.0), (30, 60.0), (1000, 29.97), (0xFFFFFFFF, 1e-300), (120000, 24.0),
                     (255 * 30, 47.0)):
        assert P.frame_length(tps, fps) == min(R.frame_length(tps, fps), 1 << 32), (tps, fps)
    assert R.frame_length(7650, 60.0) == 127 and R.frame_length(1000, 29.97) == 33


def test_numpy_restatement_equals_the_loop():
    rng = np.random.default_rng(2)
    for mode, ch in ((0, 1), (1, 3)):
        n = 1500
        e = np.zeros(n, S.EVENT_DTYPE)
        e["x"], e["y"] = rng.integers(0, 9, n), rng.integers(0, 4, n)
        e["c"] = rng.integers(0, ch, n) if ch > 1 else NONE
        e["d"] = rng.choice(np.array([0, 3, 7, 8, 127, 128, 129, 255], np.uint8), n)
        e["t"] = np.sort(rng.integers(0, 60000, n)) if mode else rng.integers(0, 900, n)
        meta = dict(width=9, height=4, channels=ch, time_mode=mode, ref_interval=255, tps=7650, source_camera=0)
        p = R.PlayerRestatement.from_meta(meta, 47.0)
        frames, bad = p.run(e, end=True)
        got, final, cur, fc = R.numpy_restate(meta, e, 47.0)
        assert bad is None and len(frames) > 5 and len(got) == len(frames)
        assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, frames))
        assert np.array_equal(final.view(np.uint64), p.display.view(np.uint64))
        assert (cur, fc) == (p.current_t, p.frame_count)


# ---- the library's schedule against the serial loop --------------------------------------------------------------

FLS = (0, 1, 3, 1 << 32)


def test_schedule_exhaustively_on_short_sequences():
    from adder_amd import player as P
    alphabet = (0, 1, 2, 3, 4, 7, 0xFFFFFFFF)
    count = 0
    assert P.schedule_host([], 1, 3).tolist() == []
    for n in range(1, 9):
        seqs = np.array(list(itertools.combinations_with_replacement(alphabet, n)), np.uint32)
        for f0 in (1, 2, 3, 4):
            for fl in FLS:
                for cur in seqs:
                    want, _ = R.serial_schedule(cur.tolist(), f0, fl)
                    got = P.schedule_host(cur, f0, fl)
                    assert got.tolist() == want, (cur.tolist(), f0, fl)
                    count += 1
    assert count > 100_000


def test_schedule_on_random_sequences_with_jumps():
    from adder_amd import player as P
    rng = np.random.default_rng(7)
    for k in range(10_000):
        n = int(rng.integers(1, 2001))
        fl = int(rng.choice([0, 1, 3, 7, 127, 255, 4250, 1 << 20, 1 << 32]))
        f0 = int(rng.integers(1, 5)) if k % 3 else int(rng.integers(1, 3000))
        step = max(fl, 1) if fl < (1 << 32) else 1 << 20
        inc = rng.integers(0, max(2, step // 3), n)  # mostly below one frame per record ...
        jumps = rng.random(n) < 0.01
        inc = np.where(jumps, rng.integers(0, 400, n) * step, inc)  # ... and jumps of many frame lengths
        cur = np.minimum(np.cumsum(inc), 0xFFFFFFFF).astype(np.uint32)
        if k % 2:
            cur[: int(rng.integers(0, n))] = 0  # nothing before the first event
        want, _ = R.serial_schedule(cur.tolist(), f0, fl)
        got = P.schedule_host(cur, f0, fl)
        assert got.tolist() == want, (k, fl, f0)


def test_the_chase_after_a_jump_gives_one_frame_per_record():
    from adder_amd import player as P
    fl = 127
    cur = np.array([0, 0] + [50 * fl + 1] * 80, np.uint32)  # 51 boundaries passed at once
    for f0 in (1, 4):
        got = P.schedule_host(cur, f0, fl).tolist()
        frames = 51 - f0  # frame_count runs from f0 up to 51, the first value with 51 * FL >= current_t
        assert got == [0, 0] + [1] * frames + [0] * (80 - frames)
        assert got == R.serial_schedule(cur.tolist(), f0, fl)[0]
    # a second jump while the chase is still going on extends it
    cur = np.array([0] + [10 * fl + 1] * 5 + [20 * fl + 1] * 40, np.uint32)
    got = P.schedule_host(cur, 1, fl).tolist()
    assert got == [0] + [1] * 20 + [0] * 25 == R.serial_schedule(cur.tolist(), 1, fl)[0]


# ---- header parser, refusals, symbols, example -------------------------------------------------------------------

@pytest.mark.parametrize("name", GOLDENS)
def test_header_parser_on_every_golden(name):
    from adder_amd import player as P
    buf = golden_bytes(name)
    meta, hb, eb = P.parse_header(buf)
    want = S.parse_header(buf)
    assert hb == want["header_size"] and eb == want["event_size"]
    for k in ("width", "height", "channels", "time_mode", "ref_interval", "tps", "source_camera"):
        assert meta[k] == want[k], k


def test_header_parser_refuses_what_is_not_a_header():
    from adder_amd import player as P, AdderHipError
    buf = bytearray(golden_bytes("bunny_v2_dt.adder")[:64])
    for bad in (b"", bytes(buf[:20]), b"xdder" + bytes(buf[5:]), bytes(buf[:5]) + b"\x09" + bytes(buf[6:])):
        with pytest.raises(AdderHipError):
            P.parse_header(bad)


def _create_code(**kw):
    from adder_amd import player as P, AdderHipError
    args = dict(width=8, height=4, channels=1, time_mode=0, ref_interval=255, tps=7650, source_camera=0)
    args.update(kw)
    try:
        P.HipPlayer(**args).close()
        return 0
    except AdderHipError as e:
        return e.code


def test_refused_cameras_and_parameters():
    for cam in (4, 5, 8, 9, 10, 1000):  # FramedF32, FramedF64, Atis, Asint: todo!() in the reference; unknown
        assert _create_code(source_camera=cam) == -1, cam
    assert _create_code(ref_interval=0) == -1
    for fps in (0.0, -1.0, float("inf"), float("nan")):
        assert _create_code(playback_fps=fps) == -1, fps
    for ch in (0, 2, 4):
        assert _create_code(channels=ch) == -1
    assert _create_code(width=0) == -1 and _create_code(out=7) == -1
    # what is accepted gets as far as the device: created, or refused for the lack of one (no CPU fallback)
    for cam in (0, 1, 2, 3, 6, 7):
        assert _create_code(source_camera=cam, playback_fps=1e9) in (0, -3)


def test_player_symbols_equal_their_binding_table():
    import adder_amd
    from adder_amd import player as P
    hdr = open(os.path.join(ROOT, "include", "adder_player.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(adder_player_\w+)\s*\(", hdr))
    assert len(names) >= 15 and names == set(P.SYMBOLS)
    adder_amd.load()
    L = ctypes.CDLL(adder_amd.LIB_PATH)
    for n in names:
        assert hasattr(L, n), n


def build_player_example(tmp_path):
    import adder_amd
    adder_amd.load()
    lib = os.path.join(ROOT, "adder-codec-rs_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "adder_play")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "examples", "adder_play.c"), "-L", lib, "-ladder_hip",
                           "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + lib,
                           "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe])
    return exe


def test_player_example_compiles_with_warnings_as_errors(tmp_path):
    assert os.path.exists(build_player_example(tmp_path))
