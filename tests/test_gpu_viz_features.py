"""Feature detection in the adder-viz player on the MI355X (include/adder_viz_player.h "Feature detection",
adder_amd.viz_player), bit for bit: the hand-derived cases (tests/viz_features_cases.py) and, against the literal
restatement (tests/viz_features_oracle.py), seeded streams on planes past a wave and past a block, limits 1, 2, 60 and
None, DeltaT and AbsoluteT with past events, in one call and in random splits; detection and the limit switched
between calls; reset; refused calls; viz_play_file and the C example with detection on."""
import os
import subprocess

import numpy as np
import pytest

import viz_features_cases as FC
import viz_player_cases as K
from framer_features_oracle import DELTA_T, ABSOLUTE_T
from viz_features_oracle import VizFeatureRestatement

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def to_device(ev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8).reshape(-1).copy()).cuda()


def host(frames):
    return frames.cpu().numpy() if hasattr(frames, "cpu") else frames


def feats(f):
    return [(int(r["index"]), int(r["t"]), int(r["x"]), int(r["y"])) for r in f]


def ivs(intervals):
    return [(int(e), [tuple(int(v) for v in p) for p in xy]) for e, xy in intervals]


class GpuImpl:
    """two contexts in lockstep behind the interface of viz_features_cases.run: one hands out POPPED frames through the
    host forms, the other RUNNING frames through the device forms; whatever does not depend on the form must agree"""

    def __init__(self, cfg, ring_frames=1024):
        from adder_amd import viz_player as V
        self.p = V.HipVizPlayer(form="popped", ring_frames=ring_frames, **cfg)
        self.r = V.HipVizPlayer(form="running", ring_frames=ring_frames, **cfg)

    def close(self):
        self.p.close()
        self.r.close()

    def detect_features(self, on):
        self.p.detect_features(on)
        self.r.detect_features(on)

    def reset(self):
        self.p.reset()
        self.r.reset()

    def set_buffer_limit(self, limit):
        self.p.set_buffer_limit(limit)
        self.r.set_buffer_limit(limit)

    def _log(self, popped, running, with_features):
        out = dict(features=feats(self.p.features()) if with_features else [], pops=[int(v) for v in self.p.pop_index],
                   intervals=ivs(self.p.frame_features()), popped=list(host(popped)), running=list(host(running)))
        out["error"] = self.p.features_error is not None
        assert out["pops"] == [int(v) for v in self.r.pop_index]
        assert out["intervals"] == ivs(self.r.frame_features())
        assert self.r.features_error == self.p.features_error
        assert not out["error"] or "where the reference panics" in self.p.features_error
        assert not with_features or out["features"] == feats(self.r.features())
        assert np.array_equal(self.p.running_intensities(), self.r.running_intensities())
        assert np.array_equal(self.p.running_frame(), self.r.running_frame())  # whichever form a call asked for
        if out["running"]:
            assert np.array_equal(out["running"][-1], self.r.running_frame())
        return out

    def ingest(self, events, bad=None):
        a = self.p.ingest(events)
        b = self.r.ingest(to_device(events) if len(events) else events)
        assert self.p.bad_index == self.r.bad_index == bad
        return self._log(a, b, True)

    def bad_event(self, events, b):
        return self.ingest(events, bad=b)

    def finish(self):
        return self._log(self.p.finish(), self.r.finish(device=True), False)

    def refused(self, kind, events, arg):
        import adder_amd as A
        before = self.state()
        for h in (self.p, self.r):
            with pytest.raises(A.AdderHipError) as ei:
                h.ingest(events, max_frames=None if kind == "refused_ring" else arg - 1)
            assert ei.value.code == A.E_OUT_CAPACITY
            assert ei.value.needed == (0 if kind == "refused_ring" else arg)
        after = self.state()
        assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))

    def state(self):
        direct = []  # the last call's features and intervals, the deque's error: as the context answers right now
        for h in (self.p, self.r):
            iv = h.frame_features()
            direct += [h.features().view(np.uint8), np.array([e for e, _ in iv], np.uint64),
                       np.array([len(xy) for _, xy in iv]), np.concatenate([xy.reshape(-1) for _, xy in iv] + [np.zeros(0, np.uint16)]),
                       np.frombuffer((h.features_error or "").encode(), np.uint8)]
        return [self.p.running_intensities(), self.p.running_frame(), self.r.running_frame(),
                np.array([self.p.frames_written, self.r.frames_written])] + direct

    def plane(self):
        return self.p.running_intensities()

    def running_frame(self):
        return self.r.running_frame()


@pytest.mark.parametrize("case", FC.CASES, ids=[c["name"] for c in FC.CASES])
def test_known_answers(case):
    g = GpuImpl(case["cfg"], ring_frames=case["ring_frames"])
    log = FC.run(g, case["ops"])
    FC.check(case, log)
    # and everything the case does not state by hand, against the restatement
    want_impl = FC.RestatementImpl(case["cfg"])
    want = FC.run(want_impl, case["ops"])
    for k, (a, b) in enumerate(zip(log, want)):
        assert a["features"] == b["features"] and a["pops"] == b["pops"] and a["intervals"] == b["intervals"], k
        assert a["error"] == b["error"], k
        for form in ("popped", "running"):
            assert len(a[form]) == len(b[form])
            for x, y in zip(a[form], b[form]):
                assert np.array_equal(np.asarray(x).reshape(-1), y), (k, form)
        assert np.array_equal(a["plane"], b["plane"]), k
    assert np.array_equal(g.running_frame().reshape(-1), want_impl.running_frame())
    g.close()


def play(cfg, ev, cuts, form, device):
    """the stream in the pieces `cuts` delimits, detection on -> features, P_j, intervals, frames, plane, running frame"""
    from adder_amd import viz_player as V
    h = V.HipVizPlayer(form=form, ring_frames=1024, **cfg)
    h.detect_features(True)
    out = dict(features=[], pops=[], intervals=[], frames=[])

    def took(frames, with_features):
        out["frames"] += list(host(frames))
        out["pops"] += [int(p) for p in h.pop_index]
        out["intervals"] += ivs(h.frame_features())
        if with_features:
            out["features"] += feats(h.features())

    for a, b in zip(cuts[:-1], cuts[1:]):
        part = ev[a:b]
        took(h.ingest(to_device(part) if device and len(part) else part), True)
        assert h.bad_index is None
    took(h.finish(device=device), False)
    out["plane"], out["running_frame"] = h.running_intensities(), h.running_frame()
    h.close()
    return out


def same(got, r, feats_want, form):
    assert got["features"] == feats(feats_want)
    assert got["pops"] == [int(p[0]) for p in r.popped]
    assert got["intervals"] == r.intervals
    col = 1 if form == "popped" else 3
    assert len(got["frames"]) == len(r.popped)
    for k, p in enumerate(r.popped):
        assert np.array_equal(got["frames"][k].reshape(-1), p[col]), (form, k)
    assert np.array_equal(got["plane"], r.running_intensities)
    assert np.array_equal(got["running_frame"].reshape(-1), r.running)


@pytest.mark.parametrize("limit", FC.LIMITS)
@pytest.mark.parametrize("time_mode", [DELTA_T, ABSOLUTE_T])
@pytest.mark.parametrize("name", list(FC.SEEDED))
def test_seeded_streams_in_one_call_and_in_random_splits(name, time_mode, limit):
    cfg, ev, r, before, f = FC.seeded(name, time_mode, limit)
    # frames pop before the drain wherever a limit forces them (on the widest plane some unit always lags behind 60)
    assert len(f) >= 5 and len(r.popped) >= 1 and (before >= 2 or limit in (60, None))
    same(play(cfg, ev, [0, len(ev)], "running", True), r, f, "running")
    same(play(cfg, ev, [0, len(ev)], "popped", False), r, f, "popped")
    rng = np.random.default_rng(13)
    cuts = K.random_splits(rng, len(ev), 7)
    assert any(a == b for a, b in zip(cuts[:-1], cuts[1:])) and any(b - a == 1 for a, b in zip(cuts[:-1], cuts[1:]))
    same(play(cfg, ev, cuts, "running", False), r, f, "running")


def test_a_split_right_after_a_pop_carries_no_last_event():
    """cuts at P + 1 for pops P of the stream: the carried event is invalid exactly there"""
    cfg, ev, r, before, f = FC.seeded("9x8", DELTA_T, 2)
    pops = sorted({int(p[0]) for p in r.popped[:before]})
    cuts = [0] + [p + 1 for p in pops[:6]] + [pops[7], pops[8] + 2, len(ev)]
    same(play(cfg, ev, cuts, "running", True), r, f, "running")


def test_switching_detection_and_the_limit_between_calls_and_reset():
    from adder_amd import viz_player as V
    cfg, ev, _, _, _ = FC.seeded("9x8", DELTA_T, 60)
    q = len(ev) // 5
    script = [("ingest", 0, q), ("detect", True), ("ingest", q, 2 * q), ("detect", False), ("ingest", 2 * q, 3 * q),
              ("detect", True), ("ingest", 3 * q, 4 * q), ("limit", 2), ("ingest", 4 * q, 5 * q), ("limit", None),
              ("detect", True), ("ingest", 5 * q, len(ev)), ("finish",)]
    h = V.HipVizPlayer(form="running", ring_frames=1024, **cfg)
    for rounds in range(2):  # the second round after reset: the state of a fresh context, the limit as it stands
        r = VizFeatureRestatement(**cfg)
        if rounds:
            h.reset()
            h.set_buffer_limit(60)
            h.detect_features(False)
            assert not h.running_intensities().any() and not h.running_frame().any() and h.frames_written == 0
        n_feat = n_cross = 0
        for op in script:
            if op[0] == "detect":
                h.detect_features(op[1]), r.detect_features(op[1])
            elif op[0] == "limit":
                h.set_buffer_limit(op[1]), r.set_buffer_limit(op[1])
            else:
                if op[0] == "ingest":
                    got, want = h.ingest(ev[op[1]:op[2]]), r.feed(ev[op[1]:op[2]])
                    assert feats(h.features()) == feats(r.last_features)
                    n_feat += len(r.last_features)
                else:
                    got, want = h.finish(), r.finish()
                assert [int(p) for p in h.pop_index] == [int(p[0]) for p in want]
                assert ivs(h.frame_features()) == r.last_intervals
                n_cross += sum(len(xy) for _, xy in r.last_intervals)
                for a, b in zip(got, want):
                    assert np.array_equal(a.reshape(-1), b[3])
                assert np.array_equal(h.running_intensities(), r.running_intensities)
                assert np.array_equal(h.running_frame().reshape(-1), r.running)
        assert n_feat >= 5 and n_cross >= 5
    h.close()


def test_with_detection_never_on_the_deque_still_runs_and_the_plane_stays_zero():
    from adder_amd import viz_player as V
    cfg, ev, _, _, _ = FC.seeded("9x8", DELTA_T, 2)
    r = VizFeatureRestatement(**cfg)
    want = r.feed(ev[:1500])
    h = V.HipVizPlayer(form="running", ring_frames=1024, **cfg)
    got = h.ingest(ev[:1500])
    assert len(got) == len(want) >= 3 and len(h.features()) == 0
    assert ivs(h.frame_features()) == r.last_intervals and all(not xy for _, xy in r.last_intervals)
    assert not h.running_intensities().any()
    for a, b in zip(got, want):
        assert np.array_equal(a.reshape(-1), b[3])
    h.close()


def test_feature_and_interval_capacity():
    import ctypes as C
    import adder_amd as A
    from adder_amd import _native as N
    cfg, ev, r, _, f = FC.seeded("9x8", DELTA_T, 2)
    g = GpuImpl(cfg)
    g.detect_features(True)
    g.p.ingest(ev)
    count = C.c_uint64(0)
    out = np.zeros(len(f), N.FRAMER_FEATURE_DTYPE)
    rc = g.p.L.adder_viz_player_features(g.p.h, out.ctypes.data, len(f) - 1, C.byref(count))
    assert rc == A.E_OUT_CAPACITY and count.value == len(f) and not out["t"].any()
    assert g.p.L.adder_viz_player_features(g.p.h, out.ctypes.data, len(f), C.byref(count)) == A.OK
    assert feats(out) == feats(f)
    pairs = C.c_uint64(0)  # a null offsets array is an argument error, not a capacity
    assert g.p.L.adder_viz_player_frame_features(g.p.h, None, None, None, 0, C.byref(pairs)) == A.E_BAD_PARAMS
    g.p.finish()  # finish has no features of its own: the last ingest call's stay
    assert feats(g.p.features()) == feats(f)
    import torch
    d_plane = torch.full(g.p.shape, 7, dtype=torch.uint8, device="cuda")  # the _device form of the plane
    assert g.p.L.adder_viz_player_running_intensities_device(g.p.h, d_plane.data_ptr(), None) == A.OK
    torch.cuda.synchronize()
    assert np.array_equal(d_plane.cpu().numpy(), g.p.running_intensities()) and d_plane.any()
    g.close()


def write_stream(path, cfg, ev):
    from oracle import oracle as O
    hdr = O.raw_header(cfg["codec_version"], cfg["width"], cfg["height"], cfg["channels"], cfg["tps"], cfg["ref_interval"],
                       cfg["delta_t_max"], source_camera=cfg["source_camera"], time_mode=cfg["time_mode"])
    open(path, "wb").write(hdr + O.raw_events(ev, cfg["channels"]) + O.raw_eof())


def file_case():
    """a framed stream whose header gives the player 30 fps: the seeded 12x9x3 stream, limit 2"""
    cfg, ev, r, _, _ = FC.seeded("12x9rgb", DELTA_T, 2)
    return cfg, ev, r


def test_viz_play_file_with_detection(tmp_path):
    from adder_amd import viz_player as V
    cfg, ev, r = file_case()
    path = str(tmp_path / "s.adder")
    write_stream(path, cfg, ev)
    got = list(V.viz_play_file(path, buffer_limit=2, detect_features=True, batch_events=1500))
    assert len(got) == len(r.popped)
    for (frame, (end_ts, xy)), p, iv in zip(got, r.popped, r.intervals):
        assert np.array_equal(frame.reshape(-1), p[3])
        assert (int(end_ts), [tuple(int(v) for v in q) for q in xy]) == iv
    plain = list(V.viz_play_file(path, buffer_limit=2, form="popped"))  # detection off: frames alone, as before
    assert all(np.array_equal(a.reshape(-1), p[1]) for a, p in zip(plain, r.popped)) and len(plain) == len(r.popped)


def test_the_c_example_with_features(tmp_path):
    import adder_amd
    adder_amd.load()
    cfg, ev, r = file_case()
    lib = os.path.join(ROOT, "adder-codec-rs_amd")
    exe, src, dst = str(tmp_path / "adder_viz_play"), str(tmp_path / "s.adder"), str(tmp_path / "out.raw")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "adder_viz_play.c"), "-L", lib, "-ladder_hip",
                           "-Wl,-rpath," + lib, "-o", exe])
    write_stream(src, cfg, ev)
    run = subprocess.run([exe, src, dst, "--limit", "2", "--features"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    got = np.fromfile(dst, np.uint8).reshape(len(r.popped), -1)
    assert np.array_equal(got, np.array([p[3] for p in r.popped]))
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("frame ")]
    assert lines == [f"frame {j}: end_ts {e}, {len(xy)} features" for j, (e, xy) in enumerate(r.intervals)]
