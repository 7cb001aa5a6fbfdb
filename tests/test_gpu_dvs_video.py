"""The DVS event video and the event-count map on the MI355X (include/adder_dvs.h, adder_amd.dvs) against the
restatement of the reference (tests/dvs_video_oracle.py): every case of tests/dvs_video_cases.py -- emitted frames
byte for byte, their indices and order, the count map, the DVS events next to a conversion with the video off --
batch splits with and without pops, the capacity refusals and what they leave behind, reset, both pop forms, a
1280x720 plane, the file tool and the C example."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import adder_stream_np as S
import dvs_oracle as R
import dvs_video_cases as K
import dvs_video_oracle as V
from test_dvs_cpu import build_example

pytestmark = pytest.mark.gpu
CASES = K.synthetic_cases() + K.golden_cases()
BY_NAME = {c["name"]: c for c in CASES}
DATE = "2024-01-02 03:04:05"


@functools.lru_cache(maxsize=None)
def want(name):
    """the restatement of a case, finished: computed once, shared, never changed"""
    c = BY_NAME[name]
    v = V.restate(c["meta"], c["tps"], c["events"], fps=c["fps"], buffer_secs=c["buffer_secs"], draw=c["draw"])
    idx, planes = v.frames()
    planes.setflags(write=False)
    return v, idx, planes, v.count_map()


def ring_of(c):
    """slots for any cut of the stream without a pop: every index up to the last one written"""
    return c["ring"] if c["golden"] is None else want(c["name"])[1][-1] + 1


def context(c, ring=None):
    from adder_amd import dvs
    h = dvs.HipDvs(**c["meta"])
    h.enable_video(c["tps"], c["fps"], c["buffer_secs"], c["draw"], ring_of(c) if ring is None else ring)
    return h


def as_list(recs):
    return list(zip(recs["t"].tolist(), recs["x"].tolist(), recs["y"].tolist(), recs["p"].tolist()))


def play(h, ev, cuts=(), pop_between=True, device=False):
    """the stream in the calls `cuts` makes of it, then finish -> (indices, planes, DVS events, bad index)"""
    idx, planes, out, bad = [], [], [], None
    edges = [0, *cuts, len(ev)]

    def take():
        i, p = h.video_pop(device=device)
        idx.extend(int(v) for v in i)
        planes.append(p.cpu().numpy() if device else p)

    for a, b in zip(edges[:-1], edges[1:]):
        out += as_list(h.convert(ev[a:b]))
        if h.bad_index is not None:
            bad = a + h.bad_index
            break
        if pop_between:
            take()
    h.video_finish()
    take()
    return idx, np.concatenate(planes), out, bad


def check(c, got):
    v, idx, planes, _ = want(c["name"])
    assert got[0] == idx
    assert got[1].shape == planes.shape and np.array_equal(got[1], planes)
    assert got[2] == v.events_out and got[3] == v.bad


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_case_equals_the_restatement(name):
    from adder_amd import dvs
    c = BY_NAME[name]
    h = context(c)
    got = play(h, c["events"])
    check(c, got)
    assert np.array_equal(h.event_count_map(), want(name)[3])
    assert np.array_equal(h.event_count_map(device=True).cpu().numpy(), want(name)[3])
    h.close()
    off = dvs.HipDvs(**c["meta"])  # the conversion with the video off: the same DVS events
    assert as_list(off.convert(c["events"])) == got[2]
    restated, _ = R.DvsRestatement.from_meta(c["meta"]).run(c["events"])
    assert restated == got[2]
    off.close()


@pytest.mark.parametrize("name", ["same_pixel", "empty_at_finish", "quiet_gap_then_restart"])
def test_every_cut_into_two_calls(name):
    c = BY_NAME[name]
    h = context(c)
    for cut in range(len(c["events"]) + 1):
        for pop_between in (True, False):
            check(c, play(h, c["events"], (cut,), pop_between))
            h.reset()  # the video starts again as well
    h.close()


@pytest.mark.parametrize("name", ["seeded_5x4x3_tm1_cam6_ref255", "seeded_33x3x1_tm0_cam0_ref255", "b0_l1",
                                  "seeded_67x5x3_tm0_cam0_ref5000", "bad_middle", "slow_unit"])
def test_random_cuts_with_and_without_pops(name):
    c = BY_NAME[name]
    rng = np.random.default_rng(len(name))
    h = context(c)
    for k in range(6):
        cuts = sorted(int(x) for x in rng.integers(0, len(c["events"]) + 1, int(rng.integers(1, 7))))
        check(c, play(h, c["events"], cuts, pop_between=k % 2 == 0, device=k % 3 == 0))
        h.reset()
    h.close()


def test_far_ahead_ring_refusal_reports_the_exact_count():
    from adder_amd import AdderHipError
    c = BY_NAME["far_ahead"]
    h = context(c, ring=1000)
    with pytest.raises(AdderHipError) as e:
        h.convert(c["events"])
    assert e.value.code == -4 and h.ring_needed == 1001
    assert h.video_ready() == 0
    # nothing was changed: the two events before the far one alone give what they give on a fresh context
    idx, planes, out, _ = play(h, c["events"][:2])
    v = V.restate(c["meta"], c["tps"], c["events"][:2], fps=c["fps"], buffer_secs=c["buffer_secs"])
    assert idx == v.frames()[0] and np.array_equal(planes, v.frames()[1]) and out == v.events_out
    h.close()
    check(c, play(context(c, ring=1001), c["events"]))


def test_ring_one_slot_short_changes_nothing():
    """unpopped frames keep their slots: the second call of two does not fit a ring one slot short of its need, is
    refused with that need, and fits once the first call's frames are popped"""
    from adder_amd import AdderHipError
    c = BY_NAME["seeded_5x4x1_tm0_cam0_ref255"]
    ev, cut = c["events"], 900
    probe = context(c)
    probe.convert(ev[:cut])
    assert probe.video_ready() > 0
    probe.convert(ev[cut:])
    need = probe.video_ring_needed()
    probe.close()
    h = context(c, ring=need - 1)
    first = as_list(h.convert(ev[:cut]))
    ready = h.video_ready()
    with pytest.raises(AdderHipError) as e:
        h.convert(ev[cut:])
    assert e.value.code == -4 and h.ring_needed == need and h.video_ready() == ready
    idx, planes = h.video_pop()
    out = first + as_list(h.convert(ev[cut:]))  # the units' state, the counts and the ring were left alone
    h.video_finish()
    i2, p2 = h.video_pop()
    check(c, ([int(v) for v in idx] + [int(v) for v in i2], np.concatenate([planes, p2]), out, None))
    assert np.array_equal(h.event_count_map(), want(c["name"])[3])
    h.close()


def test_output_capacities_one_short_leave_guards_and_state():
    from adder_amd import dvs
    c = BY_NAME["seeded_33x3x3_tm1_cam6_ref255"]
    v, idx, planes, counts = want(c["name"])
    ev = np.ascontiguousarray(c["events"], dtype=dvs.N.EVENT_DTYPE)
    h = context(c)
    L = h.L
    # the DVS output one record short: refused with the count, nothing changed
    total = len(v.events_out)
    out = np.full((total + 4) * 16, 0xA5, np.uint8)
    n_out, bad = C.c_uint64(0), C.c_uint64(0)
    rc = L.adder_dvs_convert_host(h.h, ev.ctypes.data, len(ev), dvs.OUT_EVENTS, out.ctypes.data, total - 1,
                                  C.byref(n_out), C.byref(bad))
    assert rc == -4 and n_out.value == total and np.all(out == 0xA5) and h.video_ready() == 0
    need = h.video_ring_needed()  # of the refused call, not of an earlier one
    assert need > 0
    rc = L.adder_dvs_convert_host(h.h, ev.ctypes.data, len(ev), dvs.OUT_EVENTS, out.ctypes.data, total,
                                  C.byref(n_out), C.byref(bad))
    assert rc == 0 and n_out.value == total and np.all(out[total * 16:] == 0xA5)
    assert h.video_ring_needed() == need
    assert as_list(np.frombuffer(out[: total * 16].tobytes(), dvs.DVS_EVENT_DTYPE)) == v.events_out
    h.video_finish()
    # the frames one short: refused with the count, the ready frames stay
    k = h.video_ready()
    plane = planes.shape[1] * planes.shape[2]
    assert k == len(idx)
    buf = np.full((k + 1) * plane, 0xA5, np.uint8)
    fi, got = np.full(k + 1, 0xA5A5, np.uint64), C.c_uint64(0)
    rc = L.adder_dvs_video_pop(h.h, buf.ctypes.data, k - 1, fi.ctypes.data, C.byref(got))
    assert rc == -4 and got.value == k and np.all(buf == 0xA5) and np.all(fi == 0xA5A5) and h.video_ready() == k
    import torch
    dbuf = torch.full(((k + 1) * plane,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.adder_dvs_video_pop_device(h.h, dbuf.data_ptr(), k - 1, fi.ctypes.data, C.byref(got), None)
    assert rc == -4 and got.value == k and bool((dbuf == 0xA5).all()) and h.video_ready() == k
    rc = L.adder_dvs_video_pop(h.h, buf.ctypes.data, k, fi.ctypes.data, C.byref(got))
    assert rc == 0 and got.value == k and fi[:k].tolist() == idx and fi[k] == 0xA5A5
    assert np.array_equal(buf[: k * plane].reshape(planes.shape), planes) and np.all(buf[k * plane:] == 0xA5)
    assert h.video_ready() == 0 and np.array_equal(h.event_count_map(), counts)
    h.close()


def test_enable_is_refused_after_events_and_for_bad_parameters():
    from adder_amd import dvs, AdderHipError
    c = BY_NAME["same_pixel"]
    h = dvs.HipDvs(**c["meta"])
    for kw in (dict(fps=0.0), dict(fps=float("nan")), dict(fps=float("inf")), dict(fps=-2.0), dict(tps=99)):
        with pytest.raises(AdderHipError) as e:
            h.enable_video(**dict(dict(tps=25500, fps=100.0), **kw))
        assert e.value.code == -1
    with pytest.raises(AdderHipError):
        h.video_pop()  # not enabled
    h.convert(c["events"][:2])
    with pytest.raises(AdderHipError) as e:
        h.enable_video(25500)
    assert e.value.code == -1
    h.reset()
    h.enable_video(c["tps"], c["fps"], c["buffer_secs"], c["draw"], 64)
    check(c, play(h, c["events"]))
    with pytest.raises(AdderHipError):  # finished: no more events until a reset
        h.convert(c["events"][:1])
    h.close()


def test_rgb_and_device_pop_forms_agree():
    c = BY_NAME["seeded_67x5x1_tm1_cam6_ref5000"]
    _, idx, planes, _ = want(c["name"])
    h = context(c)
    h.convert(c["events"])
    h.video_finish()
    i, rgb = h.video_pop(device=True, rgb=True)
    assert i.tolist() == idx and np.array_equal(rgb.cpu().numpy(), np.repeat(planes[..., None], 3, axis=-1))
    h.reset()
    h.convert(c["events"])
    h.video_finish()
    i, rgb = h.video_pop(rgb=True)
    assert i.tolist() == idx and np.array_equal(rgb, V.restate(c["meta"], c["tps"], c["events"], fps=c["fps"],
                                                               buffer_secs=c["buffer_secs"]).frames(rgb=True)[1])
    h.close()


def test_a_1280x720_plane_crosses_the_hand_out_grid():
    """a sparse seeded stream: its frames of 921 600 bytes, popped at once, are more 16-byte words than the
    hand-out's 2048 blocks of 256 lanes take in one pass"""
    w, h_ = 1280, 720
    rng = np.random.default_rng(77)
    px = rng.integers(0, w * h_, 300)
    rows = []
    for k in range(6000):
        p = int(px[k % 300])
        rows.append((p % w, p // w, 0xFF, 3 + (k // 300) % 7, 250))  # every unit steps a frame of 255 ticks at a time
    ev = K.events_of(rows)
    meta = K.meta_of(w, h_, cam=K.DVS_CAM)
    v = V.restate(meta, 25500, ev, fps=100.0, buffer_secs=0.05)
    idx, planes = v.frames()
    assert 10 <= len(idx) <= 40 and len(idx) * w * h_ // 16 > 2048 * 256 and v.census["drawn"] > 1000
    from adder_amd import dvs
    hd = dvs.HipDvs(**meta)
    hd.enable_video(25500, 100.0, 0.05, True, 48)
    got = play(hd, ev, (1000,), pop_between=False, device=True)
    assert got[0] == idx and np.array_equal(got[1], planes) and got[2] == v.events_out
    assert np.array_equal(hd.event_count_map(), v.count_map())
    hd.close()


def test_file_tool_and_c_example(tmp_path):
    from adder_amd import dvs
    c = BY_NAME["seeded_33x3x3_tm0_cam0_ref5000"]
    v, idx, planes, counts = want(c["name"])
    src = str(tmp_path / "in.adder")
    wire = S.write_adder(dict(c["meta"], version=2, tps=c["tps"], delta_t_max=c["tps"], adu_interval=0), c["events"])
    open(src, "wb").write(wire)
    dat = R.file_bytes(c["meta"], v.events_out, DATE)
    times = V.times_text(v.times(2.0))
    # the Python tool, in batches small enough to pop in between and with a ring that makes it cut them further
    res = dvs.adder_to_dvs_file(src, str(tmp_path / "py.dat"), date=DATE, batch_records=700,
                                video_path=str(tmp_path / "py.gray8"), counts_path=str(tmp_path / "py.counts"),
                                fps=c["fps"], buffer_secs=c["buffer_secs"], playback_slowdown=2.0, ring_frames=40)
    assert res == dict(events_in=len(c["events"]), events_out=len(v.events_out), frames=len(idx))
    assert open(tmp_path / "py.dat", "rb").read() == dat
    assert open(tmp_path / "py.gray8", "rb").read() == planes.tobytes()
    assert open(tmp_path / "py.gray8.times", "rb").read() == times
    assert open(tmp_path / "py.counts", "rb").read() == counts.tobytes()
    # without the new keywords: the same events file and nothing else
    dvs.adder_to_dvs_file(src, str(tmp_path / "plain.dat"), date=DATE)
    assert open(tmp_path / "plain.dat", "rb").read() == dat
    assert sorted(os.listdir(tmp_path)) == ["in.adder", "plain.dat", "py.counts", "py.dat", "py.gray8",
                                            "py.gray8.times"]
    # the C example
    exe = build_example(tmp_path)
    subprocess.check_call([exe, src, str(tmp_path / "c.dat"), "--date", DATE, "--video", str(tmp_path / "c.gray8"),
                           "--fps", str(c["fps"]), "--buffer-secs", str(c["buffer_secs"]), "--counts",
                           str(tmp_path / "c.counts")], timeout=120)
    assert open(tmp_path / "c.dat", "rb").read() == dat
    assert open(tmp_path / "c.gray8", "rb").read() == planes.tobytes()
    assert open(tmp_path / "c.gray8.times", "rb").read() == V.times_text(v.times())
    assert open(tmp_path / "c.counts", "rb").read() == counts.tobytes()
    subprocess.check_call([exe, src, str(tmp_path / "c0.dat"), "--date", DATE, "--video", str(tmp_path / "c0.gray8"),
                           "--fps", str(c["fps"]), "--buffer-secs", str(c["buffer_secs"]), "--no-draw"], timeout=120)
    blank = V.restate(c["meta"], c["tps"], c["events"], fps=c["fps"], buffer_secs=c["buffer_secs"], draw=False)
    assert open(tmp_path / "c0.gray8", "rb").read() == blank.frames()[1].tobytes()
    assert open(tmp_path / "c0.dat", "rb").read() == dat
