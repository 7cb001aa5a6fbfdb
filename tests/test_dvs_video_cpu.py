"""The DVS event video and the event-count map (include/adder_dvs.h) without a GPU: the census of every case of
tests/dvs_video_cases.py under the restatement (tests/dvs_video_oracle.py), hand-derived known answers of the
restatement, the library's closed-form schedule (adder_dvs_video_logic.hpp) against a serial loop exhaustively, the
count-map arithmetic, the parameter arithmetic and refusals, and the stand-alone program of the logic header."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import dvs_video_cases as K
import dvs_video_oracle as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.synthetic_cases() + K.golden_cases()


def restate(c, finish=True):
    return V.restate(c["meta"], c["tps"], c["events"], finish=finish, fps=c["fps"], buffer_secs=c["buffer_secs"],
                     draw=c["draw"])


# ---- the census ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case_reaches_its_arms(c):
    v = restate(c)
    got = dict(v.census, skipped=v.skipped())
    for key, least in c["census"].items():
        if least == 0:
            assert got.get(key, 0) == 0, (key, got)
        else:
            assert got.get(key, 0) >= least, (key, got)
    idx, planes = v.frames()
    assert idx == sorted(set(idx)) and len(planes) == len(idx) >= 1


def test_hand_built_cases_exactly():
    by = {c["name"]: c for c in CASES}
    v = restate(by["same_pixel"])
    idx, planes = v.frames()
    assert idx == [0] and planes[0, 1, 2] == 0 and planes[0, 3, 1] == 0  # the later fire wins: down, and channel 2's
    assert int((planes != 128).sum()) == 2
    v = restate(by["far_ahead"], finish=False)
    assert v.frame_count + len(v.deque) == 1001  # the ring slots one call over the whole stream needs
    v = restate(by["empty_at_finish"])
    idx, planes = v.frames()
    assert v.census["blank_at_finish"] == 1 and np.all(planes[-1] == 128) and idx[-1] == v.frame_count
    v = restate(by["nothing_pops"])
    assert v.census["pops"] == 0 and v.frames()[0] == list(range(len(v.written)))
    v = restate(by["quiet_gap_then_restart"])
    idx, _ = v.frames()
    assert v.skipped() == v.census["empty_pops"] == 98 and idx[:3] == [0, 1, 2] and idx[3] > 100
    for name, n in (("draw_off_two_blanks", 2), ("draw_off_one_blank", 1)):
        idx, planes = restate(by[name]).frames()
        assert len(idx) == n and np.all(planes == 128)
    v = restate(by["bad_middle"], finish=False)
    assert v.bad == 300 and v.census["events"] == 300
    v = restate(by["slow_unit"])
    assert v.census["late"] == 299 and len(v.events_out) == v.census["fired"] == 599  # late fires stay in the output
    v = restate(by["wrap_counts"])
    assert v.event_counts[0, 0, 0] == 3 and v.max_px_event_count == 65535
    m = v.count_map()
    assert m[0, 0, 0] == 0 and np.all(m[:, :, 1:] == 128) and np.all(m[:, :, 0] == 0)  # one channel: planes 1 and 2 stay 128


def test_sample_3_goldens_stop_at_their_bad_event_with_frames_before_it():
    by = {c["name"]: c for c in CASES}
    for name, stop in (("sample_3_ordered.adder", 332), ("sample_3_unordered.adder", 333)):
        for suffix in ("_cli_defaults", "_fps1000"):
            v = restate(by[name + suffix])
            assert v.bad == stop and v.census["events"] == stop and v.census["drawn"] > 100
            assert int(v.event_counts.sum()) == stop and len(v.written) >= 60


def test_f32_truncation_matters_in_its_case():
    assert V.frame_length(3, 0.3) == 10 and int(3 / float(np.float32(0.3))) == 9
    assert V.frame_length(25500, 29.97) == 850
    assert V.frame_length(16777217, 1.0) == 16777216  # tps as f32
    assert V.buffer_ticks(3, 1.0) == 3 and V.buffer_ticks(7650, -1.0) == 0 and V.buffer_ticks(7650, float("nan")) == 0


# ---- the library's arithmetic ---------------------------------------------------------------------------------------

def test_frame_length_and_buffer_equal_the_restatement():
    from adder_amd import dvs
    L = dvs.load()
    for tps in (1, 3, 100, 6120, 7650, 25500, 120000, 16777217, 0xFFFFFFFF):
        for x in (0.3, 1.0, 29.97, 100.0, 1000.0, 1e-3, 0.0, 1e9, 1e-30, 3.4e38):
            assert L.adder_dvs_video_frame_length(tps, x) == min(V.frame_length(tps, x), 1 << 62), (tps, x)
            assert L.adder_dvs_video_buffer_ticks(tps, x) == min(V.buffer_ticks(tps, x), 1 << 62), (tps, x)
        for x in (-1.0, float("nan"), float("-inf")):
            assert L.adder_dvs_video_buffer_ticks(tps, x) == 0
        assert L.adder_dvs_video_buffer_ticks(tps, float("inf")) == 1 << 62


def test_count_byte_on_a_grid_and_at_the_wrap():
    from adder_amd import dvs
    L = dvs.load()
    grid = list(range(0, 40)) + [127, 128, 255, 256, 1000, 65534, 65535]
    for m in grid:
        for count in grid:
            if count <= m:  # a unit's counter never passes the maximum
                assert L.adder_dvs_video_count_byte(count, m) == V.count_byte(count, m), (count, m)
    assert L.adder_dvs_video_count_byte(0, 0) == 0  # NaN as u8
    # past the wrap the counter is taken as u16 and the maximum stays 65535
    for n in (65536, 65537, 65539, 131071, 131072 + 9):
        assert L.adder_dvs_video_count_byte(n, 65535) == V.count_byte(n & 0xFFFF, 65535)


def serial(pt, fire, L, B, state, draw=True):
    """the reference's loop over one call, state = (frame_count, current_t, end)"""
    F, cur, E = state
    pop, acc, em = [], [], []
    for p, f in zip(pt, fire):
        popped = cur > F * L + B
        if popped:
            if E > F:
                em.append(F)
            F += 1
        pop.append(int(popped))
        cur = max(cur, p)
        a = bool(draw and f and f // L >= F)
        if a:
            E = max(E, f // L + 1)
        acc.append(int(a))
    return pop, acc, em, (F, cur, E)


def test_schedule_exhaustively_on_short_sequences():
    from adder_amd import dvs
    alphabet = (0, 1, 2, 3, 5, 9, 40)
    count = 0
    assert dvs.video_schedule_host([], [], 3, 1)[3] == (0, 0, 1)
    for n in range(1, 7):
        seqs = list(itertools.combinations_with_replacement(alphabet, n))  # current_t never decreases
        for L, B in ((1, 0), (1, 2), (3, 0), (3, 4), (7, 100)):
            for state in ((0, 0, 1), (2, 0, 1), (1, 6, 5), (4, 9, 2)):
                for cur in seqs:
                    # a fire at every second position, one frame behind, at, or ahead of where current_t stands
                    for shift in (0, 1, 2 * L + 1):
                        fire = [max(c, 1) + shift if k % 2 == 0 else 0 for k, c in enumerate(cur)]
                        want = serial(cur, fire, L, B, state)
                        pop, acc, em, st = dvs.video_schedule_host(cur, fire, L, B, state)
                        assert (pop.tolist(), acc.tolist(), em.tolist(), st) == want, (cur, fire, L, B, state)
                        count += 1
    assert count > 100_000


def test_schedule_on_random_sequences_with_gaps():
    from adder_amd import dvs
    rng = np.random.default_rng(5)
    empties = 0
    for k in range(3000):
        n = int(rng.integers(1, 400))
        L = int(rng.choice([1, 3, 7, 255, 4250]))
        B = int(rng.choice([0, 1, L, 10 * L]))
        pt = rng.integers(0, max(2, L // 2), n)
        pt = np.where(rng.random(n) < 0.02, rng.integers(0, 80, n) * L, pt)
        pt = np.cumsum(pt) * (rng.random(n) < 0.8)  # unit times: mostly rising, some first events (0)
        fire = np.where(rng.random(n) < 0.5, np.maximum(pt.astype(np.int64) - rng.integers(0, 20 * L, n), 0) + 1, 0)
        state = (int(rng.integers(0, 5)), int(rng.integers(0, 10 * L)), int(rng.integers(0, 8)))
        draw = k % 7 != 0
        want = serial(pt.tolist(), fire.tolist(), L, B, state, draw)
        pop, acc, em, st = dvs.video_schedule_host(pt, fire, L, B, state, draw)
        assert (pop.tolist(), acc.tolist(), em.tolist(), st) == want, (k, L, B, state)
        empties += sum(want[0]) - len(want[2])
    assert empties > 1000  # pops with an empty deque were met


def trace(c):
    """the restatement's own per-event times of a case: (restatement before finish, pt, fire_t, the frame indices
    written and frame_count before the stream's last check -- the one in front of a bad event, or finish's)"""
    v = V.DvsVideoRestatement(c["meta"], c["tps"], fps=c["fps"], buffer_secs=c["buffer_secs"], draw=c["draw"])
    pt, fire = [], []
    for e in c["events"]:
        u = (int(e["y"]), int(e["x"]), 0 if e["c"] == 0xFF else int(e["c"]))
        first, fired_before = u not in v.dvs.px, len(v.events_out)
        before = ([i for i, _ in v.written], v.frame_count)
        if v.run([e]) is not None:
            return v, pt, fire, before
        pt.append(0 if first else v.dvs.px[u][2])
        fire.append(v.events_out[-1][0] if len(v.events_out) > fired_before else 0)
    return v, pt, fire, ([i for i, _ in v.written], v.frame_count)


def finish_frames(state, L, B):
    """the stream's end as adder_dvs_video_finish takes it (dvs_video_finish of the logic header, restated)"""
    F, cur, E = state
    out = []
    if cur > F * L + B:
        if E > F:
            out.append(F)
        F += 1
    return out + (list(range(F, E)) if E > F else [F])


SHORT = [c for c in CASES if len(c["events"]) <= 12000]  # the sample_3 goldens stop at event 332 / 333


@pytest.mark.parametrize("c", SHORT, ids=[c["name"] for c in SHORT])
def test_schedule_of_a_case_in_pieces_equals_the_restatement(c):
    """the host schedule over the restatement's per-event times, the stream cut into four calls"""
    from adder_amd import dvs
    v, pt, fire, (written, frame_count) = trace(c)
    n, state, em = len(pt), (0, 0, 1), []
    for a, b in ((0, n // 3), (n // 3, n // 3), (n // 3, n - 1), (n - 1, n)):
        _, _, e, state = dvs.video_schedule_host(pt[a:b], fire[a:b], v.frame_length, v.buffer, state, c["draw"])
        em += e.tolist()
    assert em == written
    assert state[:2] == (frame_count, v.current_t)
    if state[2] > state[0]:
        assert v.deque and state[2] == v.frame_count + len(v.deque)
    # the stream's end on the library's side: one more check, then the tail
    v.finish()
    assert em + finish_frames(state, v.frame_length, v.buffer) == [i for i, _ in v.written]


# ---- refusals, the header's defaults ------------------------------------------------------------------------------------

def test_parameter_refusals():
    from adder_amd import dvs
    ok = dict(tps=25500, fps=100.0, buffer_secs=1.0)
    assert dvs.video_params_check(**ok) == (0, 255, 25500)
    for fps in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert dvs.video_params_check(**dict(ok, fps=fps))[0] == -1, fps
    assert dvs.video_params_check(tps=99, fps=100.0, buffer_secs=1.0)[0] == -1  # L == 0: the reference divides by it
    assert dvs.video_params_check(tps=0, fps=1.0, buffer_secs=1.0)[0] == -1
    assert dvs.video_params_check(tps=100, fps=100.0, buffer_secs=-3.0) == (0, 1, 0)
    assert dvs.video_params_check(tps=100, fps=100.0, buffer_secs=float("nan")) == (0, 1, 0)
    assert dvs.video_params_check(abi_version=7, **ok)[0] == -1


def test_video_params_from_header():
    from adder_amd import dvs
    from test_dvs_cpu import golden_bytes
    import adder_stream_np as S
    buf = golden_bytes("bunny_v2_dt.adder")
    p = dvs.video_params_from_header(buf)
    assert (p.tps, p.fps, p.buffer_secs, p.draw, p.ring_frames) == (S.parse_header(buf)["tps"], 100.0, 10.0, 1, 0)
    with pytest.raises(dvs.N.AdderHipError):
        dvs.video_params_from_header(b"xdder" + buf[5:])


def test_null_and_disabled_contexts_are_refused():
    from adder_amd import dvs
    L = dvs.load()
    assert L.adder_dvs_video_enable(None, None) == -1
    assert L.adder_dvs_video_finish(None) == -1
    assert L.adder_dvs_video_frames_ready(None, None) == -1
    assert L.adder_dvs_event_count_map(None, None) == -1
    assert L.adder_dvs_video_pop(None, None, 0, None, None) == -1


# ---- the stand-alone program of the logic header -------------------------------------------------------------------------

def test_logic_program_builds_and_agrees(tmp_path):
    """tests/cpu_sim/dvs_video_main.cpp: the logic header under plain g++ (also the program for host sanitizer
    builds), run over a list of schedules written here; it prints what the library's host entry gives"""
    from adder_amd import dvs
    exe = str(tmp_path / "dvs_video_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cpu_sim", "dvs_video_main.cpp"), "-o", exe])
    lines, want = [], []
    for c in SHORT:  # the case list
        v, pt, fire, (em, frame_count) = trace(c)
        lines.append(" ".join(str(x) for x in [len(pt), v.frame_length, v.buffer, int(c["draw"]), 0, 0, 1, *pt, *fire]))
        # the deque's end; a check in front of a bad event may have popped its only frame since
        e = v.frame_count + len(v.deque) if v.deque else frame_count + 1 if len(v.written) > len(em) else None
        want.append((frame_count, v.current_t, e, em))
    rng = np.random.default_rng(3)
    for k in range(40):
        n = int(rng.integers(0, 60))
        L, B = int(rng.choice([1, 3, 255])), int(rng.choice([0, 5, 700]))
        pt = np.cumsum(rng.integers(0, 2 * L + 2, n)) if n else np.zeros(0, np.int64)
        fire = np.where(rng.random(n) < 0.5, np.maximum(pt - rng.integers(0, 9 * L, n), 0) + 1, 0) if n else pt
        state = (int(rng.integers(0, 3)), int(rng.integers(0, 50)), int(rng.integers(0, 4)))
        lines.append(" ".join(str(v) for v in [n, L, B, 1, *state, *pt.tolist(), *np.asarray(fire).tolist()]))
        _, _, em, st = dvs.video_schedule_host(pt, fire, L, B, state)
        want.append((st[0], st[1], st[2], em.tolist()))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    got = [[int(x) for x in line.split()] for line in out.strip().split("\n")]
    assert len(got) == len(want)
    for g, (F, cur, E, em) in zip(got, want):
        assert g[:2] == [F, cur] and g[3] == len(em) and g[4:] == em
        assert g[2] == E if E is not None else g[2] <= F  # an empty deque: any end at or below frame_count
