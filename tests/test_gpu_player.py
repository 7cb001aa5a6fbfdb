"""The latest-event player on the MI355X (include/adder_player.h, adder_amd.player), bit for bit against the restatement
of the reference's adder_video_player (tests/player_oracle.py): the goldens, random streams, batch splits, the display
schedule's chase, the hand-out kernel's edges, capacity, bad events, the u8 output, play_file and the C example.
F64 frames are compared as uint64 bit patterns."""
import functools
import subprocess

import numpy as np
import pytest

import adder_stream_np as S
import player_oracle as R
from test_dvs_cpu import GOLDENS, golden_bytes
from test_player_cpu import build_player_example

pytestmark = pytest.mark.gpu
NONE = 0xFF
CUT = 200_000  # records of a golden that are played: the restatement of more takes more than a few seconds


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_frames(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert len(got) == len(want), (len(got), len(want))
    if len(want):
        assert np.array_equal(bits(got), bits(np.stack(want)))


def restate(meta, ev, fps, end=True):
    p = R.PlayerRestatement.from_meta(meta, fps)
    frames, bad = p.run(ev, end=end)
    return frames, p.display.copy(), (p.current_t, p.frame_count), bad


def make_player(meta, fps, out="f64"):
    from adder_amd import player as P
    return P.HipPlayer(playback_fps=fps, out=out, **meta)


def to_device(ev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8).reshape(-1).copy()).cuda()


def meta_of(w, h, ch, mode, ref=255, tps=7650, cam=0):
    return dict(width=w, height=h, channels=ch, time_mode=mode, ref_interval=ref, tps=tps, source_camera=cam)


# ---- goldens -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden_case(name, fps):
    buf = golden_bytes(name)
    meta, ev, _ = S.read_adder(buf)
    ev = ev[:CUT]  # lake_scaled_hd_out has more: its first 200 000 records are played
    pm = {k: meta[k] for k in ("width", "height", "channels", "time_mode", "ref_interval", "tps", "source_camera")}
    return buf, meta, pm, ev, restate(pm, ev, fps)


@pytest.mark.parametrize("fps", [60.0, 47.0])  # 47: FL = 162 (ref 255), 130, 2553, 6382: none divides ref_interval
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_wire_and_event_forms(name, fps):
    from adder_amd import player as P
    buf, meta, pm, ev, (want, final, clock, bad) = golden_case(name, fps)
    assert bad is None and (fps == 60.0 or pm["ref_interval"] % R.frame_length(pm["tps"], fps) != 0)
    parsed, hb, eb = P.parse_header(buf)
    assert parsed == pm
    body = buf[hb:hb + len(ev) * eb] if len(ev) == CUT else buf[hb:]
    h = P.HipPlayer.from_header(buf, playback_fps=fps)
    got = list(h.play_wire(body))
    assert h.bad_index is None and h.consumed == len(ev)
    if h.consumed == len(body) // eb:  # no EOF record among them: the stream's last check is the caller's
        got += list(h.finish().cpu().numpy())
    same_frames(np.array(got).reshape((-1,) + h.shape), want)
    assert np.array_equal(bits(h.display()), bits(final)) and h.clock() == clock
    # the AdderEvent form, device-resident, with finish
    h2 = make_player(pm, fps)
    f1 = h2.play(to_device(ev))
    f2 = h2.finish()
    same_frames(np.concatenate([f1.cpu().numpy(), f2.cpu().numpy()]), want)
    assert np.array_equal(bits(h2.display(device=True).cpu().numpy()), bits(final)) and h2.clock() == clock


# ---- random streams ----------------------------------------------------------------------------------------------

def random_stream(rng, n, w, h, ch, mode, wrap=True):
    ev = np.zeros(n, S.EVENT_DTYPE)
    ev["x"] = rng.integers(0, w, n)
    ev["y"] = rng.integers(0, h, n)
    ev["c"] = rng.integers(0, ch, n) if ch > 1 else NONE
    low = rng.integers(0, 129, n)  # 0..=128
    high = rng.integers(129, 256, n)  # 129..=255: changes nothing
    ev["d"] = np.where(rng.random(n) < 0.8, low, high)
    kind = rng.integers(0, 8, n)
    if mode == R.ABSOLUTE_T:
        t = np.cumsum(rng.integers(0, 40, n)).astype(np.uint64)  # a rising clock, with stragglers behind it
        t = np.where(kind == 1, t // 2, t)
        t = np.where(kind == 0, 0, t)
        if wrap:  # the last fifth sits just below 2^32: the round-up wraps, and so do the deltas after it
            t[-n // 5:] = (1 << 32) - 1 - rng.integers(0, 3000, n // 5)[::-1].astype(np.uint64)
    else:
        t = np.where(kind == 0, 0, rng.integers(1, 600, n)).astype(np.uint64)
        if wrap:
            t = np.where(kind == 7, (1 << 32) - rng.integers(1, 5000, n).astype(np.uint64), t)  # the sums wrap
    ev["t"] = t.astype(np.uint32)
    return ev


# FL = 0 (a rate above tps), 1, 127 (about ref / 2), 2^32 (above the stream's span: no frame at all)
RATES = [10000.0, 7650.0, 60.0, 1e-9]


@functools.lru_cache(maxsize=None)
def random_case(w, h, ch, mode, cam, fps):
    rng = np.random.default_rng([w, ch, mode, cam])
    ev = random_stream(rng, 3000, w, h, ch, mode)
    meta = meta_of(w, h, ch, mode, cam=cam)
    return meta, ev, restate(meta, ev, fps)


@pytest.mark.parametrize("cam", [0, 6])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h", [(7, 5), (257, 1)])
def test_random_streams(w, h, ch, mode, cam):
    assert [min(R.frame_length(7650, f), 1 << 32) for f in RATES] == [0, 1, 127, 1 << 32]
    for fps in RATES:
        meta, ev, (want, final, clock, bad) = random_case(w, h, ch, mode, cam, fps)
        assert bad is None and (len(want) == 0) == (fps == 1e-9) and np.any(ev["t"] == 0)
        hp = make_player(meta, fps)
        got = hp.play(ev)  # host form
        same_frames(np.concatenate([got, hp.finish().cpu().numpy()]), want)
        assert np.array_equal(bits(hp.display()), bits(final)) and hp.clock() == clock
        # the wire form, closed by an EOF record
        wire = S.write_adder(dict(meta, version=2, delta_t_max=2550, adu_interval=0), ev)
        hw = make_player(meta, fps)
        same_frames(hw.play_wire(wire[33:]), want)
        assert hw.consumed == len(ev) and hw.clock() == clock


@pytest.mark.parametrize("mode,ch,cam", [(0, 1, 0), (1, 3, 0), (1, 1, 6), (0, 3, 6)])
def test_split_invariance(mode, ch, cam):
    rng = np.random.default_rng(11 + mode + ch)
    for fps in (60.0, 7650.0):
        meta, ev, (want, final, clock, _) = random_case(7, 5, ch, mode, cam, fps)
        d = to_device(ev)
        for _ in range(2):
            cuts = np.sort(np.concatenate([rng.integers(0, len(ev), 10), [0, 0, 0, 7, 8, len(ev), len(ev)]]))
            hp = make_player(meta, fps)
            got = [hp.play(d[12 * a:12 * b]).cpu().numpy() for a, b in zip(cuts[:-1], cuts[1:])]  # 0 and 1 records too
            got.append(hp.finish().cpu().numpy())
            same_frames(np.concatenate(got), want)
            assert np.array_equal(bits(hp.display()), bits(final)) and hp.clock() == clock
        # the wire form, cut so that the EOF record is the first record of a call
        body = S.write_adder(dict(meta, version=2, delta_t_max=2550, adu_interval=0), ev)[33:]
        rb = 9 if ch == 1 else 11
        k = int(rng.integers(1, len(ev)))
        hw = make_player(meta, fps)
        got = [hw.play_wire(body[:k * rb]), hw.play_wire(body[k * rb:len(ev) * rb])]
        assert hw.consumed == len(ev) - k
        got.append(hw.play_wire(body[len(ev) * rb:]))
        assert hw.consumed == 0
        same_frames(np.concatenate(got), want)
        assert hw.clock() == clock


# ---- the schedule on the device ----------------------------------------------------------------------------------

def test_the_chase_after_a_jump_on_the_device():
    """FL = 127.  Three early events, then ONE event that moves the clock by 50 frame lengths, then 60 records of which
    every second one has d > 128.  frame_count is 1 at the jump, so the 50 checks after it each show a frame (the serial
    loop's chase), and frame k must hold exactly the events before position jump + 1 + k: the 25 valid records that
    arrive during the chase appear one by one."""
    meta = meta_of(64, 2, 1, R.ABSOLUTE_T)
    n_tail, jump = 60, 3
    ev = np.zeros(jump + 1 + n_tail, S.EVENT_DTYPE)
    ev["c"] = NONE
    ev["x"] = np.arange(len(ev))  # every record its own unit, in row 0
    ev["d"] = 7
    ev["t"][:jump] = [5, 9, 100]  # below one frame length: no frame
    ev["t"][jump] = 50 * 127 + 1
    ev["t"][jump + 1:] = 50 * 127 + 1 - np.arange(1, n_tail + 1)  # behind the clock: current_t stays
    ev["d"][jump + 2::2] = 200  # half of the tail changes nothing
    ev["x"][jump + 2::2] = 60000  # ... and may lie anywhere
    hp = make_player(meta, 60.0)
    got = hp.play(ev)
    assert len(got) == 50 and hp.clock() == (50 * 127 + 1, 51)
    value = lambda t: ((128.0 / float(t)) * 255.0) / 255.0  # a fresh unit: the event's time is its t
    for k in range(50):
        want = np.zeros((2, 64, 1))
        for i in range(jump + 1 + k):  # the display positions are consecutive
            if ev["d"][i] <= 128:
                want[0, ev["x"][i], 0] = value(ev["t"][i])
        assert np.array_equal(bits(got[k]), bits(want)), k
    same_frames(got, restate(meta, ev, 60.0, end=False)[0])
    assert len(hp.finish()) == 0


# ---- kernel edges ------------------------------------------------------------------------------------------------

def test_one_unit_plane_and_a_batch_of_one_record():
    for mode in (0, 1):
        meta = meta_of(1, 1, 1, mode)
        ev = random_stream(np.random.default_rng(mode), 400, 1, 1, 1, mode, wrap=False)
        want, final, clock, _ = restate(meta, ev, 60.0)
        hp = make_player(meta, 60.0)
        got = [hp.play(ev[i:i + 1]) for i in range(len(ev))] + [hp.finish().cpu().numpy()]
        assert all(len(g) <= 1 for g in got)
        same_frames(np.concatenate(got), want)
        assert np.array_equal(bits(hp.display()), bits(final)) and hp.clock() == clock


def test_a_run_far_longer_than_a_workgroup_and_units_without_events():
    """Unit (1, 2) receives 5 000 events in one batch (a run of 5 000 in the sorted order, about twenty workgroups of the
    per-event kernels), with display positions falling inside the run; a second unit gets a few; the other 33 units never
    receive an event and show 0.0 in every frame."""
    for mode in (0, 1):
        meta = meta_of(7, 5, 1, mode)
        rng = np.random.default_rng(5 + mode)
        n = 5040
        ev = np.zeros(n, S.EVENT_DTYPE)
        ev["x"], ev["y"], ev["c"] = 2, 1, NONE
        other = rng.choice(n, 40, replace=False)
        ev["x"][other], ev["y"][other] = 6, 4
        ev["d"] = rng.integers(0, 12, n)
        ev["t"] = np.cumsum(rng.integers(1, 9, n)) if mode else rng.integers(1, 9, n)
        want, final, clock, _ = restate(meta, ev, 60.0)
        assert len(want) > 20
        hp = make_player(meta, 60.0)
        got = np.concatenate([hp.play(to_device(ev)).cpu().numpy(), hp.finish().cpu().numpy()])
        same_frames(got, want)
        quiet = np.ones((5, 7, 1), bool)
        quiet[1, 2], quiet[4, 6] = False, False
        assert quiet.sum() == 33 and np.all(bits(got[:, quiet]) == 0)
        assert np.array_equal(bits(hp.display()), bits(final)) and hp.clock() == clock


@pytest.mark.parametrize("out", ["f64", "u8"])
def test_full_hd_plane_with_scattered_events(out):
    """1920x1080 with 5 000 scattered events and 2 frames: the hand-out's grid runs over 2 * 2 073 600 elements, past its
    edges in u (8 100 workgroups per f64 frame).  The restatement is the vectorised one (held against the loop in
    tests/test_player_cpu.py)."""
    meta = meta_of(1920, 1080, 1, R.ABSOLUTE_T)
    rng = np.random.default_rng(9)
    n = 5000
    ev = np.zeros(n, S.EVENT_DTYPE)
    ev["x"], ev["y"], ev["c"] = rng.integers(0, 1920, n), rng.integers(0, 1080, n), NONE
    ev["x"][-3:], ev["y"][-3:] = [1919, 0, 1919], [1079, 0, 0]  # the plane's corners
    ev["d"] = rng.integers(0, 10, n)
    ev["t"] = np.sort(rng.integers(1, 127, n))  # inside the first frame length ...
    ev["t"][2000] = 200  # ... but for two events that each pass a boundary
    ev["t"][4000] = 300
    want, final, cur, fc = R.numpy_restate(meta, ev, 60.0, end=True)
    assert len(want) == 2 and fc == 3
    hp = make_player(meta, 60.0, out)
    got = hp.play(to_device(ev)).cpu().numpy()
    assert len(got) == 2 and len(hp.finish()) == 0 and hp.clock() == (cur, fc)
    if out == "u8":
        assert np.array_equal(got, np.stack([R.to_u8(f) for f in want]))
        assert np.array_equal(hp.display(), R.to_u8(final))
    else:
        same_frames(got, want)
        assert np.array_equal(bits(hp.display()), bits(final))


# ---- capacity, bad events ----------------------------------------------------------------------------------------

def test_out_capacity_changes_nothing():
    import ctypes as C
    import torch
    from adder_amd import player as P
    import adder_amd._native as N
    meta, ev, (want, final, clock, _) = random_case(7, 5, 3, 1, 0, 60.0)
    first = 1000
    w1, f1, c1, _ = restate(meta, ev[:first], 60.0, end=False)
    need = len(restate(meta, ev, 60.0, end=False)[0]) - len(w1)
    assert need > 3
    hp = make_player(meta, 60.0)
    same_frames(hp.play(ev[:first]), w1)
    d = to_device(ev[first:])
    room = torch.zeros((need,) + hp.shape, dtype=torch.float64, device="cuda")
    n_frames, bad = C.c_uint64(0), C.c_uint64(0)
    rc = P.load().adder_player_play_device(hp.h, d.data_ptr(), len(ev) - first, room.data_ptr(), need - 1,
                                           C.byref(n_frames), C.byref(bad), None)
    assert rc == N.E_OUT_CAPACITY and n_frames.value == need  # one short: the count comes back ...
    assert hp.clock() == c1 and np.array_equal(bits(hp.display()), bits(f1))  # ... and nothing has changed
    assert not room.any()
    with pytest.raises(N.AdderHipError) as ei:
        hp.play(d, max_frames=need - 1)
    assert ei.value.code == N.E_OUT_CAPACITY and ei.value.needed == need and hp.clock() == c1
    got = hp.play(d, max_frames=need)  # with room: the full result
    same_frames(np.concatenate([got.cpu().numpy(), hp.finish().cpu().numpy()]), want[len(w1):])
    assert np.array_equal(bits(hp.display()), bits(final)) and hp.clock() == clock


@pytest.mark.parametrize("field,value", [("x", 7), ("y", 5), ("c", 3)])
def test_a_bad_event_mid_batch(field, value):
    from adder_amd import player as P
    meta, base, _ = random_case(7, 5, 3, 0, 0, 60.0)
    k = 1234
    ev = base.copy()
    ev[field][k], ev["d"][k] = value, 7  # on the bound: the first coordinate outside the plane
    want, final, clock, bad = restate(meta, ev, 60.0, end=False)
    assert bad == k
    hp = make_player(meta, 60.0)
    got = hp.play(ev)
    assert hp.bad_index == k
    same_frames(got, want)
    assert np.array_equal(bits(hp.display()), bits(final)) and hp.clock() == clock
    # identical to a batch that ends there
    h2 = make_player(meta, 60.0)
    same_frames(h2.play(ev[:k]), want)
    assert h2.clock() == clock and h2.bad_index is None
    # the following call continues as if the event had been left out
    rest = hp.play(ev[k + 1:])
    w_all, f_all, c_all, _ = restate(meta, np.concatenate([ev[:k], ev[k + 1:]]), 60.0, end=False)
    same_frames(np.concatenate([got, rest]), w_all)
    assert np.array_equal(bits(hp.display()), bits(f_all)) and hp.clock() == c_all
    # a record with d > 128 outside the plane is no bad event
    ev["d"][k] = 255
    w3, _, c3, bad3 = restate(meta, ev, 60.0, end=False)
    h3 = make_player(meta, 60.0)
    same_frames(h3.play(ev), w3)
    assert bad3 is None and h3.bad_index is None and h3.clock() == c3


# ---- u8 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ref,tie,rounded", [(255, 127.5, 128), (253, 126.5, 126)])
def test_u8_is_the_rounded_f64_with_ties_to_even(ref, tie, rounded):
    """The value of a fresh unit's event is ((2^d / t) * ref) / 255, so 255 * value = ref * 2^d / t up to rounding.  With
    t a power of two the quotient is exact: d = 0, t = 2 gives ref / 2 = 127.5 (ref 255: between 127 and the even 128) or
    126.5 (ref 253: between the even 126 and 127).  The test asserts that the f64 run really holds these ties.  Values
    above 1.0 (small t) saturate at 255."""
    meta = meta_of(16, 4, 1, R.ABSOLUTE_T, ref=ref)
    rng = np.random.default_rng(ref)
    n = 600
    ev = np.zeros(n, S.EVENT_DTYPE)
    ev["x"], ev["y"], ev["c"] = rng.integers(0, 16, n), rng.integers(1, 4, n), NONE  # row 0 is kept for the four below
    ev["d"] = rng.integers(0, 9, n)
    ev["t"] = np.cumsum(rng.integers(0, 30, n))
    ev[:4] = np.array([(0, 0, NONE, 0, 0, 2), (1, 0, NONE, 3, 0, 16), (2, 0, NONE, 9, 0, 1), (3, 0, NONE, 128, 0, 3)],
                      S.EVENT_DTYPE)  # two ties, one value far above 1.0, one 0.0
    f64 = make_player(meta, 60.0).play(ev)
    u8 = make_player(meta, 60.0, "u8").play(ev)
    assert len(f64) > 10 and u8.dtype == np.uint8
    scaled = f64[-1] * 255.0
    assert scaled[0, 0, 0] == tie and scaled[0, 1, 0] == tie and scaled[0, 2, 0] > 255.0
    assert u8[-1][0, 0, 0] == rounded and u8[-1][0, 2, 0] == 255 and u8[-1][0, 3, 0] == 0
    assert np.array_equal(u8, np.clip(np.rint(f64 * 255), 0, 255).astype(np.uint8))


# ---- play_file and the C example ---------------------------------------------------------------------------------

@pytest.mark.parametrize("out", ["f64", "u8"])
def test_play_file_halves_a_batch_that_shows_too_many_frames(tmp_path, out):
    import adder_amd as A
    from adder_amd import player as P
    name = "sample_3_unordered.adder"
    buf, meta, pm, ev, (want, _, _, _) = golden_case(name, 60.0)
    src = tmp_path / name
    src.write_bytes(buf)
    calls = []
    real = P.HipPlayer.play_wire
    P.HipPlayer.play_wire = lambda self, rec, **kw: (calls.append(len(rec) // self.record_bytes), real(self, rec, **kw))[1]
    try:
        # batches of 700 records show up to ~33 frames: more than the 8 a batch may show, so they are halved
        got = list(A.play_file(str(src), 60.0, out=out, batch_events=700, max_batch_frames=8))
    finally:
        P.HipPlayer.play_wire = real
    assert len(want) == 499 and min(calls) < 700 // 2 and max(calls) == 700
    if out == "u8":
        assert np.array_equal(np.stack(got), np.stack([R.to_u8(f) for f in want]))
    else:
        same_frames(np.stack(got), want)


@pytest.mark.parametrize("flags", [[], ["--fps", "47"], ["--u8", "--frames", "3"]])
def test_c_example_matches_the_restatement(tmp_path, flags):
    exe = build_player_example(tmp_path)
    fps = 47.0 if "--fps" in flags else 60.0
    for name in ("lake_scaled_hd_out.adder.gz", "sample_3_ordered.adder", "bunny_v2_t.adder"):
        buf, meta, pm, ev, (want, _, clock, _) = golden_case(name, fps)
        src = tmp_path / name.replace(".gz", "")
        body_end = meta["header_size"] + len(ev) * meta["event_size"]
        src.write_bytes(buf[:body_end] if len(ev) == CUT else buf)  # the same cut as the restatement's
        dst = tmp_path / (src.name + ".raw")
        r = subprocess.run([exe, str(src), str(dst)] + flags, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        frames = np.stack(want)
        data = R.to_u8(frames).tobytes() if "--u8" in flags else frames.tobytes()
        assert dst.read_bytes() == data, name
        assert f"{len(ev)} ADDER events -> {len(want)} frames (current_t {clock[0]})" in r.stdout
