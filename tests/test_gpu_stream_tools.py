"""Stream migration and adder-info on the MI355X (include/adder_stream.h, adder_amd.stream_tools), byte for byte and
bit for bit against the restatement (tests/stream_tools_oracle.py): the goldens through every entry point, random
streams, batch splits, the transcoder's own output migrated in HBM, round trips, the three error kinds, the file
tools and the C example."""
import os
import struct
import subprocess

import numpy as np
import pytest

import adder_stream_np as S
import stream_tools_oracle as R
from test_stream_tools_cpu import DVS_CAM, GOLDENS, build_example, golden_bytes, lib_meta

pytestmark = pytest.mark.gpu


def bits(x):
    return struct.pack("<d", x)


def to_array(out):
    ev = np.zeros(len(out), S.EVENT_DTYPE)
    if len(out):
        a = np.array(out, dtype=np.int64)
        ev["x"], ev["y"], ev["c"], ev["d"], ev["t"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4]
    return ev


def restate_migration(meta, ev, out_mode):
    out, bad = R.Migration(meta, out_mode).run(ev)
    return to_array(out), bad


def restate_info(meta, ev):
    r = R.Info(meta)
    bad = r.run(ev)
    return r, bad


def other_mode(meta):
    return R.DELTA_T if R.in_time_mode(meta) == R.ABSOLUTE_T else R.ABSOLUTE_T


def migrator(meta, out_mode):
    from adder_amd import stream_tools as T
    return T.HipStreamMigrator(out_time_mode=out_mode, **lib_meta(meta))


def informer(meta):
    from adder_amd import stream_tools as T
    return T.HipStreamInfo(**lib_meta(meta))


def body_of(meta, ev):
    return S.write_adder(meta, ev, close=False)[len(S.build_header(meta)):]


def device_bytes(t):
    return t.cpu().numpy().tobytes()


def migrate_every_way(meta, ev, out_mode, want):
    """event and wire entry points, host and device forms, out of place and in place -> all equal `want`"""
    import torch
    n = len(want)
    got = migrator(meta, out_mode).migrate(ev)
    assert np.array_equal(got, want)
    d = torch.from_numpy(ev.view(np.uint8).copy()).cuda()
    keep = d.clone()
    h = migrator(meta, out_mode)
    out = h.migrate(d)
    assert device_bytes(out)[: 12 * n] == want.tobytes() and torch.equal(d, keep)
    h = migrator(meta, out_mode)
    h.migrate(d, out=d)
    assert device_bytes(d)[: 12 * n] == want.tobytes()
    wire, want_wire = body_of(meta, ev), body_of(meta, want)
    h = migrator(meta, out_mode)
    assert h.migrate_wire(wire) == want_wire and h.consumed == len(ev)
    dw = torch.frombuffer(bytearray(wire), dtype=torch.uint8).cuda() if len(wire) else torch.empty(0, dtype=torch.uint8).cuda()
    h = migrator(meta, out_mode)
    out = h.migrate_wire(dw)
    assert device_bytes(out)[: len(want_wire)] == want_wire and device_bytes(dw) == wire
    h = migrator(meta, out_mode)
    h.migrate_wire(dw, out=dw)
    assert device_bytes(dw)[: len(want_wire)] == want_wire


def info_every_way(meta, ev, want):
    import torch
    for how in ("host", "device", "wire_host", "wire_device"):
        h = informer(meta)
        if how == "host":
            got = h.fold(ev)
        elif how == "device":
            got = h.fold(torch.from_numpy(ev.view(np.uint8).copy()).cuda())
        elif how == "wire_host":
            got = h.fold_wire(body_of(meta, ev))
        else:
            got = h.fold_wire(torch.frombuffer(bytearray(body_of(meta, ev)), dtype=torch.uint8).cuda())
        assert (bits(got[0]), bits(got[1]), got[2]) == (bits(want.min), bits(want.max), want.count), how


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_migration_round_trip_and_info(name):
    from adder_amd import stream_tools as T
    buf = golden_bytes(name)
    meta, ev, _ = S.read_adder(buf)
    out_mode = other_mode(meta)
    want, bad = restate_migration(meta, ev, out_mode)
    assert bad is None and len(want) == len(ev)
    migrate_every_way(meta, ev, out_mode, want)
    # and back: the identity for version >= 1; a v0 stream comes back as the restatement says (it is not rounded up
    # on the way out and is on the way back)
    back_meta = dict(meta, version=max(meta["version"], 2), time_mode=out_mode)
    back = migrator(back_meta, other_mode(back_meta)).migrate(want)
    want_back, bad = restate_migration(back_meta, want, other_mode(back_meta))
    assert bad is None and np.array_equal(back, want_back)
    if meta["version"] >= 1:
        assert np.array_equal(back, ev)
    r, bad = restate_info(meta, ev)
    assert bad is None
    info_every_way(meta, ev, r)
    h = T.HipStreamInfo.from_header(buf)
    h.fold_wire(buf[meta["header_size"]:])
    assert h.consumed == len(ev)
    assert h.report(meta["header_size"], len(buf), h.consumed) == \
        R.report(meta, meta["header_size"], len(buf), len(ev), True, r.min, r.max)


def random_stream(rng, n, w, h, ch, absolute, big_t, hot=True, ref=255, cam=0):
    """a few units with thousands of events and many with one; D_EMPTY, d == 128 and t == 0 mixed in.  absolute:
    the AbsoluteT stream migrate_v2 makes of it for this ref and camera, so that its units' times do not decrease
    (and respect the round-up of a framed camera)"""
    ev = np.zeros(n, S.EVENT_DTYPE)
    units = rng.integers(0, w * h * ch, n)
    if hot:
        units = np.where(rng.random(n) < 0.6, rng.integers(0, 3, n), units)
    ev["c"] = units % ch if ch > 1 else 0xFF
    ev["x"] = (units // ch) % w
    ev["y"] = units // ch // w
    ev["d"] = rng.choice(np.array([0, 1, 2, 3, 5, 7, 8, 9, 12, 20, 40, 100, 127, 128, 128, 255, 255], np.uint8), n)
    t = np.where(rng.integers(0, 5, n) == 0, 0, rng.integers(1, 3000, n)).astype(np.int64)
    if big_t:  # the first event of some units starts close to 2^32
        first = np.unique(units, return_index=True)[1]
        first = first[rng.random(len(first)) < 0.5]
        t[first] = (1 << 32) - rng.integers(30_000_000, 40_000_000, len(first))
    ev["t"] = t.astype(np.uint32)
    if absolute:
        meta = dict(width=w, height=h, channels=ch, version=2, time_mode=0, ref_interval=ref, source_camera=cam)
        ev, bad = restate_migration(meta, ev, R.ABSOLUTE_T)
        assert bad is None
    return ev


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("cam", [0, DVS_CAM])
@pytest.mark.parametrize("ref", [1, 255, 5000])
@pytest.mark.parametrize("version,time_mode", [(0, 0), (1, 0), (2, 0), (2, 1), (3, 1)])
def test_fuzz(ch, cam, ref, version, time_mode):
    rng = np.random.default_rng(ch * 100000 + cam * 10000 + ref * 10 + version * 2 + time_mode)
    w, h = 7, 5
    absolute = time_mode == 1
    ev = random_stream(rng, 9000, w, h, ch, absolute, big_t=True, ref=ref, cam=cam)
    meta = dict(width=w, height=h, channels=ch, version=version, time_mode=time_mode, ref_interval=ref,
                source_camera=cam, tps=ref * 30, delta_t_max=ref * 30, adu_interval=0)
    out_mode = other_mode(meta)
    want, bad = restate_migration(meta, ev, out_mode)
    assert bad is None and int(want["t"].max() if out_mode == 1 else ev["t"].max()) > (1 << 32) - 40_000_000
    migrate_every_way(meta, ev, out_mode, want)
    back_meta = dict(meta, version=max(version, 2), time_mode=out_mode)
    back = migrator(back_meta, other_mode(back_meta)).migrate(want)
    if version >= 1:
        assert np.array_equal(back, ev)
    else:
        assert np.array_equal(back, restate_migration(back_meta, want, other_mode(back_meta))[0])
    r, bad = restate_info(meta, ev)
    assert bad is None
    info_every_way(meta, ev, r)
    # pass-through modes leave the events alone
    for mode in (R.MIXED, R.in_time_mode(meta)):
        assert np.array_equal(migrator(meta, mode).migrate(ev), ev)


def test_fold_arms_on_the_device():
    """the hand-made streams of the CPU file: d == 128 raising min, t == 0, the sticky zero, D_EMPTY in AbsoluteT, an
    event that lowers min and would have raised max"""
    N = 0xFF
    cases = [([(0, 0, N, 3, 4), (0, 0, N, 3, 2), (0, 0, N, 0, 1)], 0),
             ([(0, 0, N, 0, 4), (0, 0, N, 128, 2), (0, 0, N, 0, 1)], 0),
             ([(0, 0, N, 128, 0), (0, 0, N, 5, 1)], 0), ([(0, 0, N, 128, 0)], 0), ([(0, 0, N, 254, 1)], 0),
             ([(0, 0, N, 0, 4), (0, 0, N, 200, 7), (0, 0, N, 0, 8), (0, 0, N, 128, 2), (0, 0, N, 3, 1)], 0),
             ([(0, 0, N, 0, 100), (0, 0, N, 255, 300), (0, 0, N, 1, 400)], 1),
             ([(0, 0, N, 0, 100), (1, 0, N, 0, 100), (0, 0, N, 0, 300)], 1), ([(0, 0, N, 255, 9)], 0)]
    for events, tm in cases:
        meta = dict(width=2, height=1, channels=1, version=2, time_mode=tm, ref_interval=255, source_camera=0,
                    tps=1, delta_t_max=1, adu_interval=0)
        ev = to_array(events)
        r, bad = restate_info(meta, ev)
        assert bad is None
        info_every_way(meta, ev, r)


def test_split_invariance():
    import torch
    rng = np.random.default_rng(21)
    for ch, version, time_mode, cam in ((1, 2, 0, 0), (3, 2, 1, 0), (1, 1, 0, DVS_CAM), (3, 3, 1, DVS_CAM)):
        ev = random_stream(rng, 6000, 5, 4, ch, time_mode == 1, big_t=False, cam=cam)
        meta = dict(width=5, height=4, channels=ch, version=version, time_mode=time_mode, ref_interval=255,
                    source_camera=cam, tps=7650, delta_t_max=7650, adu_interval=0)
        out_mode = other_mode(meta)
        want, bad = restate_migration(meta, ev, out_mode)
        assert bad is None
        r, _ = restate_info(meta, ev)
        for _ in range(3):
            cuts = np.sort(np.concatenate([rng.integers(0, len(ev), 12), [0, 0, 7, 8, len(ev), len(ev)]]))
            hm, hi = migrator(meta, out_mode), informer(meta)
            d = torch.from_numpy(ev.view(np.uint8).copy()).cuda()
            for a, b in zip(cuts[:-1], cuts[1:]):  # empty batches and batches of one event included
                hm.migrate(d[12 * a:12 * b], out=d[12 * a:12 * b])
                got = hi.fold(ev[a:b])
            assert device_bytes(d) == want.tobytes()
            assert (bits(got[0]), bits(got[1]), got[2]) == (bits(r.min), bits(r.max), r.count)
            # the wire forms, split
            hm, hi = migrator(meta, out_mode), informer(meta)
            wire, rb, out = body_of(meta, ev), (9 if ch == 1 else 11), b""
            for a, b in zip(cuts[:-1], cuts[1:]):
                out += hm.migrate_wire(wire[rb * a:rb * b])
                got = hi.fold_wire(wire[rb * a:rb * b])
            assert out == body_of(meta, want)
            assert (bits(got[0]), bits(got[1]), got[2]) == (bits(r.min), bits(r.max), r.count)


def test_the_three_error_kinds_and_eof_in_the_middle():
    rng = np.random.default_rng(5)
    w, h = 4, 3
    base_meta = dict(width=w, height=h, channels=1, version=2, ref_interval=5000, source_camera=0, tps=1,
                     delta_t_max=1, adu_interval=0)
    # forward: a sum above u32::MAX; outside the plane
    ev = random_stream(rng, 900, w, h, 1, False, big_t=False, hot=False)
    meta = dict(base_meta, time_mode=0)
    over = ev.copy()
    over["t"][400] = (1 << 32) - 5
    nxt = 401 + int(np.nonzero((over["x"][401:] == over["x"][400]) & (over["y"][401:] == over["y"][400]))[0][0])
    over["t"][nxt] = 77
    outside = ev.copy()
    outside["x"][500] = w
    for bad_ev, k in ((over, None), (outside, 500)):
        want, bad = restate_migration(meta, bad_ev, R.ABSOLUTE_T)
        assert bad is not None and (k is None or bad == k) and (k is not None or bad in (400, nxt))
        hm = migrator(meta, R.ABSOLUTE_T)
        got = hm.migrate(bad_ev)
        assert hm.bad_index == bad and np.array_equal(got, want)
        # the state holds the events before `bad` and nothing after: the rest continues as if it had been left out
        rest = hm.migrate(bad_ev[bad + 1:])
        whole, bad2 = restate_migration(meta, np.concatenate([bad_ev[:bad], bad_ev[bad + 1:]]), R.ABSOLUTE_T)
        assert bad2 is None and hm.bad_index is None and np.array_equal(np.concatenate([got, rest]), whole)
        r, ibad = restate_info(meta, bad_ev)
        hi = informer(meta)
        got = hi.fold(bad_ev)
        assert hi.bad_index == ibad and (bits(got[0]), bits(got[1]), got[2]) == (bits(r.min), bits(r.max), r.count)
    # inverse and AbsoluteT info: a time below the unit's previous one
    ev = random_stream(rng, 900, w, h, 1, True, big_t=False, hot=False, ref=5000)
    meta = dict(base_meta, time_mode=1)
    assert restate_migration(meta, ev, R.DELTA_T)[1] is None
    late = ev.copy()
    prev = 600 - 1 - int(np.nonzero(((late["x"][:600] == late["x"][600]) & (late["y"][:600] == late["y"][600]))[::-1])[0][0])
    assert late["t"][prev] > 0
    late["t"][600] = late["t"][prev] - 1
    want, bad = restate_migration(meta, late, R.DELTA_T)
    assert bad == 600
    hm = migrator(meta, R.DELTA_T)
    got = hm.migrate(late)
    assert hm.bad_index == 600 and np.array_equal(got, want)
    rest = hm.migrate(late[601:])
    whole, bad2 = restate_migration(meta, np.concatenate([late[:600], late[601:]]), R.DELTA_T)
    assert bad2 is None and np.array_equal(np.concatenate([got, rest]), whole)
    r, ibad = restate_info(meta, late)
    hi = informer(meta)
    got = hi.fold(late)
    assert ibad == 600 and hi.bad_index == 600
    assert (bits(got[0]), bits(got[1]), got[2]) == (bits(r.min), bits(r.max), r.count)
    r2 = R.Info(meta)
    assert r2.run(np.concatenate([late[:600], late[601:]])) is None
    got = hi.fold(late[601:])
    assert (bits(got[0]), bits(got[1]), got[2]) == (bits(r2.min), bits(r2.max), r2.count)
    # an EOF record in the middle of a wire batch: 9-byte and 11-byte records
    for ch in (1, 3):
        meta = dict(base_meta, time_mode=0, channels=ch)
        ev = random_stream(rng, 300, w, h, ch, False, big_t=False)
        rb = 9 if ch == 1 else 11
        wire = bytearray(body_of(meta, ev))
        wire[rb * 120:rb * 120 + 4] = b"\xff\xff\xff\xff"
        want, _ = restate_migration(meta, ev[:120], R.ABSOLUTE_T)
        hm = migrator(meta, R.ABSOLUTE_T)
        assert hm.migrate_wire(bytes(wire)) == body_of(meta, want) and hm.consumed == 120 and hm.bad_index is None
        hi = informer(meta)
        r, _ = restate_info(meta, ev[:120])
        got = hi.fold_wire(bytes(wire))
        assert hi.consumed == 120 and (bits(got[0]), bits(got[1]), got[2]) == (bits(r.min), bits(r.max), 120)


def transcode(W, H, C, T, time_mode):
    """The transcoder on the device in PixelMultiMode::Normal: (uint8 CUDA tensor of its AdderEvents, their count)."""
    import torch
    import adder_amd as A
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.empty((T, W * H * C), dtype=torch.uint8, device="cuda")
    A.synth_clip_device(d_frames, A.CONTENT_SCENE, W, H, C, num_frames=T, stream=st)
    hv = A.HipVideo(W, H, C, time_mode=time_mode, multi_mode=A.MULTI_NORMAL, ref_time=255, delta_t_max=255 * 4)
    hv.update_crf(0)
    d_events = torch.empty(12 * 4 * W * H * C * T, dtype=torch.uint8, device="cuda")
    d_offsets = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv.integrate_device(d_frames, d_events, d_offsets, stream=st)
    n = hv.finish()
    torch.cuda.synchronize()
    return d_events[: 12 * n].clone(), n


@pytest.mark.parametrize("W,H,C,T", [(320, 180, 1, 24), (320, 180, 3, 24), (1920, 1080, 1, 60)])
def test_transcoder_output_migrated_in_hbm(W, H, C, T):
    """a DeltaT stream of the transcoder, migrated on the device, is its AbsoluteT stream, and the other way round"""
    import torch
    from adder_amd import stream_tools as T_
    d_dt, n_dt = transcode(W, H, C, T, 0)
    d_abs, n_abs = transcode(W, H, C, T, 1)
    assert n_dt == n_abs > W * H * C
    for d in (d_dt, d_abs):  # Normal mode emits no D_EMPTY event: the condition under which the reference agrees
        assert int((d.view(-1, 12)[:, 5] == 255).sum()) == 0
    kw = dict(codec_version=2, ref_interval=255, source_camera=0)
    fwd = T_.HipStreamMigrator(W, H, C, time_mode=0, out_time_mode=1, **kw)
    out = fwd.migrate(d_dt)
    assert fwd.bad_index is None and torch.equal(out, d_abs)
    inv = T_.HipStreamMigrator(W, H, C, time_mode=1, out_time_mode=0, **kw)
    out = inv.migrate(d_abs)
    assert inv.bad_index is None and torch.equal(out, d_dt)
    # in place, in 4 batches that split units' runs
    fwd.reset()
    work = d_dt.clone()
    cuts = [0, n_dt // 5, n_dt // 2, n_dt // 2 + 1, n_dt]
    for a, b in zip(cuts[:-1], cuts[1:]):
        fwd.migrate(work[12 * a:12 * b], out=work[12 * a:12 * b])
    assert torch.equal(work, d_abs)
    # the fold sees the same relative times in both streams
    if W == 320:  # the fold of both streams against the restatement (AbsoluteT: relative to the raw previous time)
        for d, tm in ((d_dt, 0), (d_abs, 1)):
            got = T_.HipStreamInfo(W, H, C, time_mode=tm, **kw).fold(d)
            ev = np.frombuffer(d.cpu().numpy().tobytes(), S.EVENT_DTYPE)
            r, bad = restate_info(dict(width=W, height=H, channels=C, version=2, time_mode=tm), ev)
            assert bad is None
            assert (bits(got[0]), bits(got[1]), got[2]) == (bits(r.min), bits(r.max), n_dt)


@pytest.mark.parametrize("name", ["nyc_v1_1px.adder", "virat_small_gray.adder", "sample_3_ordered.adder",
                                  "adder_info_test_sample.adder"])
def test_file_tools_and_c_example(tmp_path, name):
    import adder_amd as A
    exe = build_example(tmp_path)
    buf = golden_bytes(name)
    meta, ev, _ = S.read_adder(buf)
    src = tmp_path / name
    src.write_bytes(buf)
    for word, mode in (("absolute", 1), ("delta_t", 0), ("mixed", 2)):
        want, bad = restate_migration(meta, ev, mode)
        assert bad is None
        expect = R.migrated_header(buf, mode) + body_of(meta, want) + R.EOF
        dst = tmp_path / f"{word}.adder"
        assert A.migrate_file(str(src), str(dst), word, batch_records=1000) == dict(events=len(ev))
        assert dst.read_bytes() == expect
        cdst = tmp_path / f"{word}_c.adder"
        r = subprocess.run([exe, str(src), str(cdst), word], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == "Done!\n", r.stdout + r.stderr
        assert cdst.read_bytes() == expect
    r, _ = restate_info(meta, ev)
    assert A.adder_info_file(str(src), True, batch_records=777) == \
        R.report(meta, meta["header_size"], len(buf), len(ev), True, r.min, r.max)
    assert A.adder_info_file(str(src)) == R.report(meta, meta["header_size"], len(buf), len(ev))
    if name == "nyc_v1_1px.adder":
        gold = golden_bytes("nyc_source_v2_2_1px.adder")
        assert (tmp_path / "absolute.adder").read_bytes()[: 33 + 45] == gold[: 33 + 45]
    if name == "adder_info_test_sample.adder":
        text = A.adder_info_file(str(src), True)
        assert "event count: 141" in text and "Events per pixel channel: 35" in text and "6.2792 dB" in text


def test_file_tools_report_a_bad_event_and_refuse_compressed_input(tmp_path):
    import adder_amd as A
    buf = golden_bytes("virat_small_gray.adder")
    meta, ev, _ = S.read_adder(buf)
    ev = ev.copy()
    ev["x"][5000] = meta["width"]
    src = tmp_path / "bad.adder"
    src.write_bytes(S.write_adder(meta, ev))
    want, bad = restate_migration(meta, ev, R.DELTA_T)
    assert bad == 5000
    with pytest.raises(A.AdderHipError) as ei:
        A.migrate_file(str(src), str(tmp_path / "out.adder"), "delta_t", batch_records=1024)
    assert ei.value.code == -20 and ei.value.index == 5000
    assert (tmp_path / "out.adder").read_bytes() == R.migrated_header(buf, 0) + body_of(meta, want) + R.EOF
    with pytest.raises(A.AdderHipError) as ei:
        A.adder_info_file(str(src), True, batch_records=1024)
    assert ei.value.index == 5000
    comp = tmp_path / "c.adder"
    comp.write_bytes(buf[:23] + b"\x00" + buf[24:])  # not a raw stream's event size
    with pytest.raises(A.AdderHipError):
        A.adder_info_file(str(comp))
