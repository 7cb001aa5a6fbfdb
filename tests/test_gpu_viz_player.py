"""The adder-viz player on the MI355X (include/adder_viz_player.h, adder_amd.viz_player), bit for bit against the literal
restatement of `consume` (tests/viz_player_oracle.py) in both output forms and in P_j, and in the popped form against
the committed C checker directly: planes past a block and past a wave, long single-unit runs, silent units and rows,
batch splits (empty, one record, inside a cascade), a lowered limit, no limit against HipFramer, capacity, bad
events, wire input, viz_play_file on a golden and the C example."""
import functools
import os
import subprocess

import numpy as np
import pytest

import adder_stream_np as S
import viz_player_cases as K
from viz_player_oracle import VizRestatement, DELTA_T, ABSOLUTE_T, EVENT_DTYPE
from test_dvs_cpu import golden_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFF


def restate(cfg, ev, finish=True):
    r = VizRestatement(**cfg)
    r.feed(ev)
    before = len(r.popped)
    if finish:
        r.finish()
    return r, before


def to_device(ev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8).reshape(-1).copy()).cuda()


def play(cfg, ev, cuts=None, form="popped", device=False, wire=False, finish=True, ring_frames=1024):
    """-> (frames [n, units], P_j) of the stream fed in the pieces `cuts` delimits"""
    from adder_amd import viz_player as V
    from oracle import oracle as O
    h = V.HipVizPlayer(form=form, ring_frames=ring_frames, **cfg)
    cuts = [0, len(ev)] if cuts is None else cuts
    frames, pops = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        part = ev[a:b]
        if wire:
            body = np.frombuffer(O.raw_events(part, cfg["channels"]), np.uint8)
            got = h.ingest_wire(to_device(body) if device else body)
            assert h.consumed == len(part)
        else:
            got = h.ingest(to_device(part) if device and len(part) else part)
        assert h.bad_index is None
        frames += list(got.cpu().numpy() if hasattr(got, "cpu") else got)
        pops += list(h.pop_index)
    if finish:
        got = h.finish(device=device)
        frames += list(got.cpu().numpy() if hasattr(got, "cpu") else got)
        pops += list(h.pop_index)
    n_units = cfg["width"] * cfg["height"] * cfg["channels"]
    h.close()
    return np.array(frames, np.uint8).reshape(-1, n_units), [int(p) for p in pops]


def same(got, want_popped, form):
    frames, pops = got
    assert pops == [p[0] for p in want_popped]
    assert len(frames) == len(want_popped)
    col = 1 if form == "popped" else 3
    for k, w in enumerate(want_popped):
        assert np.array_equal(frames[k], w[col]), (form, k)


# ---- planes, streams, forms ----------------------------------------------------------------------------------------

PLANES = {  # width, height, channels, events, generator options
    "1x1": (1, 1, 1, 300, {}),
    "7x5": (7, 5, 1, 3000, dict(silent_units=0.15)),  # units that never fire: their rows only ever get forced
    "4x3rgb": (4, 3, 3, 3000, {}),
    "257x3": (257, 3, 1, 5000, {}),  # a row longer than a 256-thread block
    "3x70": (3, 70, 1, 5000, {}),  # more rows than a wave has lanes
    "3x70-silent-rows": (3, 70, 1, 5000, dict(silent_rows=(5, 69))),  # two rows never fire: nothing pops before finish
}


@functools.lru_cache(maxsize=None)
def plane_case(name, time_mode, limit):
    w, h, c, n, opts = PLANES[name]
    cfg = K.base_cfg(w, h, c, time_mode=time_mode, buffer_limit=limit,
                     source_camera=K.DVS if name == "4x3rgb" else K.FRAMED_U8, output_fps=47.0 if name == "7x5" else 30.0)
    ev = K.gen_sweep(1, w, h, c, n, time_mode=time_mode, past=0.1 if time_mode == ABSOLUTE_T else 0.0,
                     slow_rows=0.3 if h < 10 else 0.03, **opts)
    if "silent_units" in opts:
        assert len(np.unique(ev["y"].astype(np.int64) * w + ev["x"])) < w * h
    r, before = restate(cfg, ev)
    return cfg, ev, r, before


@pytest.mark.parametrize("time_mode", [DELTA_T, ABSOLUTE_T])
@pytest.mark.parametrize("name", list(PLANES))
def test_planes_both_forms_and_the_c_checker(name, time_mode):
    cfg, ev, r, before = plane_case(name, time_mode, 2)
    if name == "3x70-silent-rows":
        assert before == 0 and len(r.popped) >= 3
    else:  # pops before the drain, Nones among them
        assert before >= 3 and (name == "1x1" or any(not p[2].all() for p in r.popped[:before]))
    got = play(cfg, ev, form="popped", device=True)
    same(got, r.popped, "popped")
    want_c = K.c_checker_frames(ev, cfg)  # the committed C checker, directly
    assert got[1] == [p for p, _ in want_c]
    for k, (_, b) in enumerate(want_c):
        assert np.array_equal(got[0][k], b), k
    same(play(cfg, ev, form="running"), r.popped, "running")


@pytest.mark.parametrize("limit", [1, 60, None])
def test_other_limits(limit):
    cfg, ev, r, _ = plane_case("7x5", DELTA_T, limit)
    same(play(cfg, ev, form="running", device=True), r.popped, "running")
    same(play(cfg, ev, form="popped"), r.popped, "popped")


def test_a_long_run_of_one_unit():
    """5 000 events of one unit among a few of the others: one thread walks the run, the others' rows stall or force"""
    cfg = K.base_cfg(3, 2, 1, buffer_limit=3)
    rng = np.random.default_rng(5)
    ev = np.zeros(5000, EVENT_DTYPE)
    ev["x"], ev["y"], ev["c"], ev["d"] = 1, 1, NONE, rng.integers(0, 9, 5000)
    ev["t"] = rng.integers(1, 120, 5000)
    others = K.gen_stream(6, 3, 2, 1, 60, max_step=2)
    at = np.sort(rng.choice(5000, 60, replace=False))
    ev[at] = others
    r, before = restate(cfg, ev)
    assert before >= 10
    # the unit runs ~4 900 frames ahead inside the one call: a ring that holds them
    same(play(cfg, ev, form="running", device=True, ring_frames=8192), r.popped, "running")
    same(play(cfg, ev, form="popped", device=True, ring_frames=8192), r.popped, "popped")


# ---- splits ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["7x5", "3x70"])
def test_random_splits_give_the_same_frames(name):
    cfg, ev, r, _ = plane_case(name, DELTA_T, 2)
    rng = np.random.default_rng(11)
    cuts = K.random_splits(rng, len(ev), 9)
    assert any(a == b for a, b in zip(cuts[:-1], cuts[1:])) and any(b - a == 1 for a, b in zip(cuts[:-1], cuts[1:]))
    same(play(cfg, ev, cuts, form="running", device=True), r.popped, "running")
    same(play(cfg, ev, cuts, form="popped"), r.popped, "popped")


def test_a_split_right_after_the_event_that_starts_a_cascade():
    cfg, ev, r, before = plane_case("7x5", DELTA_T, 60)
    pops = [p[0] for p in r.popped[:before]]
    runs = [p for p in set(pops) if pops.count(p) >= 3]
    assert runs  # a cascade of at least three frames
    e = min(runs)
    for cut in (e, e + 1):  # the call ends before / with the event: the cascade belongs to the call that holds it
        same(play(cfg, ev, [0, cut, len(ev)], form="running"), r.popped, "running")


def test_lowering_the_limit_between_calls_pops_at_the_opening():
    from adder_amd import viz_player as V
    cfg, ev, _, _ = plane_case("7x5", DELTA_T, 60)
    cut = len(ev) // 2
    r = VizRestatement(**cfg)
    r.feed(ev[:cut])
    n1 = len(r.popped)
    r.set_buffer_limit(1)
    r.feed(ev[cut:])
    opening = [p for p in r.popped[n1:] if p[0] == cut - 1]
    assert opening  # the loop in front of the read loop popped with the new limit
    r.finish()
    h = V.HipVizPlayer(form="running", ring_frames=1024, **cfg)
    got = list(h.ingest(ev[:cut]))
    pops = list(h.pop_index)
    h.set_buffer_limit(1)
    got += list(h.ingest(ev[cut:]))
    pops += list(h.pop_index)
    got += list(h.finish())
    pops += list(h.pop_index)
    same((np.array(got).reshape(len(got), -1), [int(p) for p in pops]), r.popped, "running")
    assert np.array_equal(h.running_frame().reshape(-1), r.running)


# ---- no limit: the exact framer's frames ---------------------------------------------------------------------------------

def test_no_limit_gives_hipframer_frames():
    import adder_amd as A
    cfg = K.base_cfg(5, 4, 1, buffer_limit=None)
    ev = K.gen_stream(77, 5, 4, 1, 1500, lag_rows=0.0, max_step=2)  # every unit fires, none lags far
    frames, _ = play(cfg, ev, form="popped", device=True, finish=False)
    fr = A.HipFramer(cfg["width"], cfg["height"], cfg["channels"], tps=cfg["tps"], ref_interval=cfg["ref_interval"],
                     delta_t_max=cfg["delta_t_max"], output_fps=cfg["output_fps"], codec_version=cfg["codec_version"],
                     time_mode=cfg["time_mode"], source_camera=cfg["source_camera"], ring_frames=1024)
    fr.ingest(ev)
    want = np.frombuffer(fr.pop(), np.uint8).reshape(-1, frames.shape[1])
    # the player pops a complete frame when an event completes it; the framer hands the same frames out afterwards
    assert len(want) == len(frames) >= 20
    assert np.array_equal(frames, want)


# ---- refusals --------------------------------------------------------------------------------------------------------

def test_capacity_one_short_changes_nothing():
    import adder_amd as A
    from adder_amd import viz_player as V
    cfg, ev, r, before = plane_case("4x3rgb", DELTA_T, 2)
    h = V.HipVizPlayer(form="popped", ring_frames=1024, **cfg)
    with pytest.raises(A.AdderHipError) as ei:
        h.ingest(ev, max_frames=before - 1)
    assert ei.value.code == A.E_OUT_CAPACITY and ei.value.needed == before and h.frames_written == 0
    got = h.ingest(ev, max_frames=before)  # nothing changed: the same call with room
    same((np.array(got).reshape(before, -1), [int(p) for p in h.pop_index]), r.popped[:before], "popped")


@pytest.mark.parametrize("field,value", [("x", 7), ("y", 5), ("c", 1)])
def test_a_bad_event_commits_what_came_before(field, value):
    import adder_amd as A
    from adder_amd import viz_player as V
    cfg, ev, _, _ = plane_case("7x5", DELTA_T, 2)
    b = 1234
    bad = ev.copy()
    bad[field][b] = value
    r, before = restate(cfg, ev[:b], finish=False)
    h = V.HipVizPlayer(form="running", ring_frames=1024, **cfg)
    got = h.ingest(to_device(bad))
    assert h.bad_index == b
    same((got.cpu().numpy().reshape(len(got), -1), [int(p) for p in h.pop_index]), r.popped, "running")
    rest = ev[b:]  # the stream goes on as if the batch had ended before b
    r.feed(rest)
    r.finish()
    more = list(h.ingest(rest)) + list(h.finish())
    assert np.array_equal(np.array(more).reshape(len(more), -1), np.array([p[3] for p in r.popped[before:]]))


def test_limit_zero_is_refused():
    import adder_amd as A
    from adder_amd import viz_player as V
    with pytest.raises(A.AdderHipError) as ei:
        V.HipVizPlayer(**K.base_cfg(2, 2, 1, buffer_limit=0))
    assert ei.value.code == A.E_BAD_PARAMS
    h = V.HipVizPlayer(**K.base_cfg(2, 2, 1, buffer_limit=2))
    with pytest.raises(A.AdderHipError):
        h.set_buffer_limit(0)


def test_a_unit_past_the_ring_is_refused_and_changes_nothing():
    import adder_amd as A
    from adder_amd import viz_player as V
    cfg = K.base_cfg(2, 1, 1, buffer_limit=None)
    h = V.HipVizPlayer(ring_frames=4, form="popped", **cfg)
    ev = np.zeros(2, EVENT_DTYPE)
    ev[0] = (0, 0, NONE, 3, 0, 255 * 5)  # frames 0..4: one more than the ring holds
    ev[1] = (1, 0, NONE, 3, 0, 255)
    with pytest.raises(A.AdderHipError) as ei:
        h.ingest(ev)
    assert ei.value.code == A.E_OUT_CAPACITY and ei.value.needed == 0
    ev[0]["t"] = 255 * 4
    assert len(h.ingest(ev)) == 1 and h.frames_written == 1


# ---- wire input, the golden, the example -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["7x5", "4x3rgb"])
def test_wire_input(name):
    cfg, ev, r, _ = plane_case(name, DELTA_T, 2)
    cuts = [0, len(ev) // 3, len(ev)]
    same(play(cfg, ev, cuts, form="running", wire=True, device=True), r.popped, "running")
    same(play(cfg, ev, cuts, form="popped", wire=True), r.popped, "popped")


def test_wire_input_stops_at_the_eof_record():
    from adder_amd import viz_player as V
    from oracle import oracle as O
    cfg, ev, r, _ = plane_case("7x5", DELTA_T, 2)
    n = 2000
    body = O.raw_events(ev[:n], 1) + O.raw_eof() + O.raw_events(ev[n:n + 50], 1)  # records after it are not looked at
    want, _ = restate(cfg, ev[:n])
    h = V.HipVizPlayer(form="running", ring_frames=1024, **cfg)
    got = list(h.ingest_wire(to_device(np.frombuffer(body, np.uint8)))), list(h.pop_index)
    assert h.consumed == n and h.bad_index is None
    more = list(h.finish(device=True).cpu().numpy())
    frames = [f.cpu().numpy() for f in got[0]] + more
    same((np.array(frames).reshape(len(frames), -1), [int(p) for p in got[1]] + [int(p) for p in h.pop_index]),
         want.popped, "running")


CUT = 200_000


@functools.lru_cache(maxsize=None)
def lake(limit):
    from adder_amd import viz_player as V
    buf = golden_bytes("lake_scaled_hd_out.adder.gz")
    meta, ev, _ = S.read_adder(buf)
    ev = ev[:CUT]
    fps = V.reconstructed_frame_rate(meta["tps"], meta["ref_interval"], meta["source_camera"])
    cfg = K.base_cfg(meta["width"], meta["height"], meta["channels"], time_mode=meta["time_mode"],
                     source_camera=meta["source_camera"], buffer_limit=limit, tps=meta["tps"],
                     ref_interval=meta["ref_interval"], delta_t_max=meta["delta_t_max"], output_fps=fps,
                     codec_version=meta["version"])
    return buf, cfg, ev, K.c_checker_frames(ev, cfg)


def _running(cfg, popped_c, ev):
    """the running frames from the restatement (it keeps the Option masks the C checker's bytes do not show)"""
    r, _ = restate(cfg, ev)
    assert [p[0] for p in r.popped] == [p for p, _ in popped_c]
    return r


@pytest.mark.parametrize("limit", [60, 2])
def test_viz_play_file_on_the_lake_golden(limit, tmp_path):
    from adder_amd import viz_player as V
    buf, cfg, ev, want_c = lake(limit)
    path = str(tmp_path / "lake.adder")
    open(path, "wb").write(buf)
    got = list(V.viz_play_file(path, buffer_limit=limit, form="popped", max_records=CUT, batch_events=70_000))
    assert len(got) == len(want_c) and len(got) >= 3
    for k, (_, b) in enumerate(want_c):
        assert np.array_equal(got[k].reshape(-1), b), k
    if limit == 2:  # the running form, against the restatement
        r = _running(cfg, want_c, ev)
        run = list(V.viz_play_file(path, buffer_limit=limit, form="running", max_records=CUT))
        assert np.array_equal(np.array(run).reshape(len(run), -1), np.array([p[3] for p in r.popped]))


def build_viz_example(tmp_path):
    import adder_amd
    adder_amd.load()
    lib = os.path.join(ROOT, "adder-codec-rs_amd")
    exe = str(tmp_path / "adder_viz_play")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "adder_viz_play.c"), "-L", lib, "-ladder_hip",
                           "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_the_c_example_on_the_lake_golden(tmp_path):
    buf, cfg, ev, want_c = lake(2)
    exe = build_viz_example(tmp_path)
    src, dst = str(tmp_path / "lake.adder"), str(tmp_path / "out.raw")
    open(src, "wb").write(buf)
    r = subprocess.run([exe, src, dst, "--limit", "2", "--popped", "--records", str(CUT)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dst, np.uint8).reshape(len(want_c), -1)
    assert np.array_equal(got, np.array([b for _, b in want_c]))
