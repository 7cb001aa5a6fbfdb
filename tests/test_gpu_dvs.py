"""ADDER -> DVS on the MI355X (include/adder_dvs.h, adder_amd.dvs), byte for byte against the restatement of the
reference's adder-to-dvs (tests/dvs_oracle.py): the device log1p, the goldens in binary / text / reorder modes, random
streams, batch splits, device-resident transcoder output, a 1080p sample, bad events and the C example."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import adder_stream_np as S
import dvs_oracle as R
from test_dvs_cpu import DVS_CAM, GOLDENS, build_example, golden_bytes, _sweep_args

pytestmark = pytest.mark.gpu
DATE = "2024-01-02 03:04:05"


def as_list(recs):
    return list(zip(recs["t"].tolist(), recs["x"].tolist(), recs["y"].tolist(), recs["p"].tolist()))


def restate(meta, events, theta=0.01):
    return R.DvsRestatement.from_meta(meta, theta).run(events)


def test_device_log1p_equals_the_host_routine_bit_for_bit():
    from adder_amd import dvs
    x = _sweep_args()
    got = dvs.log1p_device(x)
    want = dvs.log1p(x)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", [g for g in GOLDENS if not g.startswith("sample_3")])
def test_goldens_binary_text_and_reorder(name):
    from adder_amd import dvs
    buf = golden_bytes(name)
    meta, ev, _ = S.read_adder(buf)
    want, bad = restate(meta, ev)
    assert bad is None
    _, hb, eb = dvs.parse_header(buf)
    body = buf[hb:]
    h = dvs.HipDvs.from_header(buf)
    got = h.convert_wire(body, dvs.OUT_EVENTS)  # text: the full time
    assert h.bad_index is None and h.consumed == len(ev)
    assert as_list(got) == want
    assert dvs.format_text(got) == R.text_bytes(want)
    h.reset()
    dat = h.convert_wire(body, dvs.OUT_DAT)
    assert dat.tobytes() == R.dat_bytes(want)
    srt = h.sort(dat, dvs.OUT_DAT)
    assert srt.tobytes() == R.dat_bytes(R.reorder(want))
    assert np.all(np.diff(srt["t"].astype(np.int64)) >= 0)
    # the AdderEvent form of the same stream, device-resident
    import torch
    h2 = dvs.HipDvs.from_header(buf)
    d = torch.from_numpy(ev.view(np.uint8).copy()).cuda()
    out = h2.convert(d, dvs.OUT_EVENTS)
    assert as_list(np.frombuffer(out.cpu().numpy().tobytes(), dvs.DVS_EVENT_DTYPE)) == want


@pytest.mark.parametrize("name,stop", [("sample_3_ordered.adder", 332), ("sample_3_unordered.adder", 333)])
def test_sample_3_stops_at_the_d_254_event(name, stop):
    """unit (9, 3) carries d = 254 after its first event: the reference panics there (D_SHIFT[254])"""
    from adder_amd import dvs
    buf = golden_bytes(name)
    meta, ev, _ = S.read_adder(buf)
    want, bad = restate(meta, ev)
    assert bad == stop and ev["d"][stop] == 254
    _, hb, _ = dvs.parse_header(buf)
    h = dvs.HipDvs.from_header(buf)
    got = h.convert_wire(buf[hb:], dvs.OUT_EVENTS)
    assert h.bad_index == stop and as_list(got) == want


def random_stream(rng, n, w, h, ch, big_t):
    ev = np.zeros(n, S.EVENT_DTYPE)
    ev["x"] = rng.integers(0, w, n)
    ev["y"] = rng.integers(0, h, n)
    ev["c"] = rng.integers(0, ch, n) if ch > 1 else 0xFF
    ev["d"] = rng.choice(np.array([0, 1, 2, 3, 5, 7, 8, 9, 12, 20, 40, 127, 128, 255], np.uint8), n)
    kind = rng.integers(0, 4, n)
    t = np.where(kind == 0, 0, rng.integers(1, 3000, n)).astype(np.uint64)
    if big_t:
        t = np.where(kind == 3, (1 << 32) - rng.integers(1, 5000, n).astype(np.uint64), t)
    ev["t"] = t.astype(np.uint32)
    seen = set()
    for i in range(n):  # a unit's first event has d <= 128 (255 only later)
        u = (int(ev["x"][i]), int(ev["y"][i]), int(ev["c"][i]))
        if u not in seen:
            seen.add(u)
            if ev["d"][i] == 255:
                ev["d"][i] = 6
    return ev


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("time_mode", [0, 1])
@pytest.mark.parametrize("cam", [0, DVS_CAM])
@pytest.mark.parametrize("ref", [255, 5000])
def test_fuzz(ch, time_mode, cam, ref):
    from adder_amd import dvs
    rng = np.random.default_rng(ch * 1000 + time_mode * 100 + cam * 10 + ref)
    w, h = 6, 5
    ev = random_stream(rng, 6000, w, h, ch, big_t=True)
    meta = dict(width=w, height=h, channels=ch, time_mode=time_mode, ref_interval=ref, source_camera=cam)
    for theta in (0.01, 0.0, 0.3):
        want, bad = restate(meta, ev, theta)
        assert bad is None
        hd = dvs.HipDvs(theta=theta, **meta)
        got = hd.convert(ev, dvs.OUT_EVENTS)
        assert as_list(got) == want, (theta, len(got), len(want))
        # the same through the wire form
        hw = dvs.HipDvs(theta=theta, **meta)
        wire = S.write_adder(dict(meta, version=2, tps=ref * 30, delta_t_max=ref * 30, adu_interval=0), ev)
        _, hb, _ = dvs.parse_header(wire)
        dat = hw.convert_wire(wire[hb:], dvs.OUT_DAT)
        assert hw.consumed == len(ev) and dat.tobytes() == R.dat_bytes(want)


def test_split_invariance():
    from adder_amd import dvs
    import torch
    rng = np.random.default_rng(11)
    for ch, time_mode, cam in ((1, 0, 0), (3, 1, 0), (1, 1, DVS_CAM)):
        ev = random_stream(rng, 5000, 5, 4, ch, big_t=True)
        meta = dict(width=5, height=4, channels=ch, time_mode=time_mode, ref_interval=255, source_camera=cam)
        want, _ = restate(meta, ev)
        one = as_list(dvs.HipDvs(**meta).convert(ev))
        assert one == want
        for _ in range(3):
            cuts = np.sort(np.concatenate([rng.integers(0, len(ev), 12), [0, 0, 7, 8, len(ev), len(ev)]]))
            hd = dvs.HipDvs(**meta)
            d = torch.from_numpy(ev.view(np.uint8).copy()).cuda()
            got = []
            for a, b in zip(cuts[:-1], cuts[1:]):  # empty batches and batches of one event included
                out = hd.convert(d[12 * a:12 * b], dvs.OUT_EVENTS)
                got += as_list(np.frombuffer(out.cpu().numpy().tobytes(), dvs.DVS_EVENT_DTYPE))
            assert got == one


def test_wide_plane_packs_x_unmasked():
    from adder_amd import dvs
    meta = dict(width=20000, height=2, channels=1, time_mode=0, ref_interval=255, source_camera=DVS_CAM)
    ev = np.zeros(4, S.EVENT_DTYPE)
    ev["x"], ev["y"], ev["c"], ev["d"], ev["t"] = [19999, 16500, 19999, 16500], [1, 0, 1, 0], 0xFF, [7, 7, 8, 5], 100
    want, _ = restate(meta, ev)
    assert len(want) == 2
    dat = dvs.HipDvs(**meta).convert(ev, dvs.OUT_DAT)
    assert dat.tobytes() == R.dat_bytes(want)


def test_bad_events_and_capacity():
    import ctypes as C
    from adder_amd import dvs
    import adder_amd._native as N
    rng = np.random.default_rng(3)
    meta = dict(width=4, height=3, channels=1, time_mode=0, ref_interval=255, source_camera=0)
    base = random_stream(rng, 800, 4, 3, 1, big_t=False)
    for k, mutate in ((300, dict(d=200)), (500, dict(x=9)), (650, dict(y=3))):
        ev = base.copy()
        for f, v in mutate.items():
            ev[f][k] = v
        want, bad = restate(meta, ev)
        assert bad == k
        hd = dvs.HipDvs(**meta)
        got = hd.convert(ev)
        assert hd.bad_index == k and as_list(got) == want
        # the state holds the events before k and nothing after: the rest continues as if k had been left out
        rest = as_list(hd.convert(ev[k + 1:]))
        want_all, _ = restate(meta, np.concatenate([ev[:k], ev[k + 1:]]))
        assert want + rest == want_all
    # a unit's first event with D_EMPTY (unit (4, 2) of a wider plane turns up first at index 100)
    meta5 = dict(meta, width=5)
    ev = base.copy()
    ev["x"][100], ev["y"][100], ev["d"][100] = 4, 2, 255
    want, bad = restate(meta5, ev)
    assert bad == 100
    hd = dvs.HipDvs(**meta5)
    got = hd.convert(ev)
    assert hd.bad_index == 100 and as_list(got) == want
    # capacity: nothing changes, the required count comes back
    import torch
    d = torch.from_numpy(base.view(np.uint8).copy()).cuda()
    want, _ = restate(meta, base)
    hd = dvs.HipDvs(**meta)
    n_out, badi = C.c_uint64(0), C.c_uint64(0)
    out = torch.empty(16 * len(base), dtype=torch.uint8, device="cuda")
    rc = dvs.load().adder_dvs_convert_device(hd.h, d.data_ptr(), len(base), dvs.OUT_EVENTS, out.data_ptr(), 3,
                                             C.byref(n_out), C.byref(badi), None)
    assert rc == N.E_OUT_CAPACITY and n_out.value == len(want) > 3
    got = hd.convert(d)
    assert as_list(np.frombuffer(got.cpu().numpy().tobytes(), dvs.DVS_EVENT_DTYPE)) == want


def transcode(W, H, C, T, time_mode, content):
    """The transcoder on the device (adder_hip_integrate_device) and the CPU oracle's events of the same clip."""
    import torch
    import adder_amd as A
    from oracle import oracle as O
    clip = O.synth_clip(content, W, H, C, T)
    ov = O.Video(W, H, C, time_mode=time_mode, multi_mode=O.COLLAPSE, ref_time=255, delta_t_max=255 * 4)
    ov.set_crf_parameters(0, 10)
    ov.reset_c_thresh(0)
    want = np.concatenate([ov.integrate_matrix(f) for f in clip])
    hv = A.HipVideo(W, H, C, time_mode=time_mode, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=255 * 4)
    hv.update_crf(0)
    d_frames = torch.from_numpy(clip.reshape(T, -1)).cuda()
    d_events = torch.empty(12 * 4 * W * H * C * T, dtype=torch.uint8, device="cuda")
    d_offsets = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv.integrate_device(d_frames, d_events, d_offsets, stream=torch.cuda.current_stream().cuda_stream)
    n = hv.finish()
    return d_events[: 12 * n], want


@pytest.mark.parametrize("C,time_mode", [(1, 0), (1, 1), (3, 0)])
def test_device_end_to_end(C, time_mode):
    from adder_amd import dvs
    from oracle import oracle as O
    d_events, oracle_events = transcode(320, 180, C, 24, time_mode, O.CONTENT_SCENE)
    meta = dict(width=320, height=180, channels=C, time_mode=time_mode, ref_interval=255, source_camera=0)
    want, bad = restate(meta, oracle_events)
    assert bad is None and len(want) > 1000
    hd = dvs.HipDvs(**meta)
    out = hd.convert(d_events, dvs.OUT_DAT)
    assert out.cpu().numpy().tobytes() == R.dat_bytes(want)


def test_scale_1080p_sample_of_units():
    """1080p x 300 scene frames, transcoded and converted on the device; ~2000 units checked against the
    restatement of the device's own events for those units."""
    import torch
    import adder_amd as A
    from adder_amd import dvs
    W, H, T = 1920, 1080, 300
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.empty((T, W * H), dtype=torch.uint8, device="cuda")
    A.synth_clip_device(d_frames, A.CONTENT_SCENE, W, H, 1, num_frames=T, stream=st)
    d_ev = torch.empty((int(W * H * T * 0.75) + 1024, 3), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv = A.HipVideo(W, H, 1, time_mode=A.TIME_DELTA_T, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=255)
    hv.update_crf(0)
    hv.integrate_device(d_frames, d_ev, d_off, stream=st)
    n = hv.finish()
    del d_frames
    assert n > 10_000_000
    ev = d_ev[:n]
    hd = dvs.HipDvs(W, H, 1, time_mode=0, ref_interval=255, source_camera=0)
    out = hd.convert(ev.view(torch.uint8).reshape(-1), dvs.OUT_EVENTS).view(torch.int32).reshape(-1, 4)
    assert hd.bad_index is None
    rng = np.random.default_rng(7)
    sample = torch.zeros(W * H, dtype=torch.bool, device="cuda")
    units = rng.choice(W * H, 2000, replace=False)
    sample[torch.from_numpy(units).cuda()] = True
    ex, ey = ev[:, 0] & 0xFFFF, (ev[:, 0] >> 16) & 0xFFFF
    mine = ev[sample[(ey * W + ex).long()]].cpu().numpy().copy().view(S.EVENT_DTYPE).reshape(-1)
    ox, oy = out[:, 2] & 0xFFFF, (out[:, 2] >> 16) & 0xFFFF
    got = out[sample[(oy * W + ox).long()]].cpu().numpy().copy().view(dvs.DVS_EVENT_DTYPE).reshape(-1)
    want, bad = R.DvsRestatement(W, H, 1, 0, 255, 0).run(mine)
    assert bad is None and len(want) > 1000
    assert as_list(got) == want


@pytest.mark.parametrize("flags", [[], ["--text"], ["--reorder"], ["--theta", "0.05"]])
def test_c_example_matches_the_restatement(tmp_path, flags):
    exe = build_example(tmp_path)
    for name in ("lake_scaled_hd_out.adder.gz", "virat_small_gray.adder", "bunny_v2_t.adder", "sample_3_ordered.adder"):
        src = tmp_path / name.replace(".gz", "")
        src.write_bytes(golden_bytes(name))
        dst = tmp_path / (src.name + ".dat")
        r = subprocess.run([exe, str(src), str(dst), "--date", DATE] + flags, capture_output=True, text=True)
        meta, ev, _ = S.read_adder(src.read_bytes())
        theta = float(flags[1]) if flags[:1] == ["--theta"] else 0.01
        want, bad = restate(meta, ev, theta)
        assert r.returncode == (0 if bad is None else 1), r.stdout + r.stderr
        assert dst.read_bytes() == R.file_bytes(meta, want, DATE, text="--text" in flags,
                                                 reorder_="--reorder" in flags, bad=bad), name


@pytest.mark.parametrize("text,reorder", [(False, False), (True, False), (False, True)])
def test_adder_to_dvs_file(tmp_path, text, reorder):
    import adder_amd as A
    for name in ("lake_scaled_hd_out.adder.gz", "sample_3_unordered.adder"):
        src = tmp_path / name.replace(".gz", "")
        src.write_bytes(golden_bytes(name))
        dst = tmp_path / "out"
        meta, ev, _ = S.read_adder(src.read_bytes())
        want, bad = restate(meta, ev)
        if bad is None:
            res = A.adder_to_dvs_file(str(src), str(dst), text=text, reorder=reorder, date=DATE, batch_records=7777)
            assert res == dict(events_in=len(ev), events_out=len(want))
        else:
            with pytest.raises(A.AdderHipError) as ei:
                A.adder_to_dvs_file(str(src), str(dst), text=text, reorder=reorder, date=DATE, batch_records=100)
            assert ei.value.code == -16 and ei.value.index == bad
        assert dst.read_bytes() == R.file_bytes(meta, want, DATE, text=text, reorder_=reorder, bad=bad)
