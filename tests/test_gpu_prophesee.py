"""Prophesee .dat -> ADDER on the device (include/adder_prophesee.h, adder_amd.prophesee) against the restatement of
the reference (tests/prophesee_oracle.py) and the C++ mirror (host_py.prophesee): byte for byte, for any split of the
record stream, from host and device records, to raw and compressed files, with every error rule."""
import math
import os

import numpy as np
import pytest

import prophesee_oracle as R
from adder_amd import prophesee as P
from adder_amd import _native as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def recording(seed, W, H, n, span=300000, t0=2, hot=0.05, hot_share=0.3, disorder=0.02, burst=True):
    """Seeded camera records: hot pixels, bursts at one t, out-of-order t; the last record one tick after the
    largest t, so the end assert holds."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(t0, t0 + span, n)).astype(np.int64)
    if burst and n > 100:
        a = int(rng.integers(0, n - 50))
        t[a:a + 40] = t[a]
    k = int(n * disorder)
    if k:
        i = rng.integers(0, n, k)
        t[i] = np.maximum(t[i] - rng.integers(0, 5000, k), 0)
    units = W * H
    hot_px = rng.choice(units, max(1, int(units * hot)), replace=False)
    px = rng.integers(0, units, n)
    m = rng.random(n) < hot_share
    px[m] = hot_px[rng.integers(0, len(hot_px), int(m.sum()))]
    x, y = px % W, px // W
    p = rng.integers(0, 2, n)
    t = np.append(t, t.max() + 1)
    x, y, p = np.append(x, 0), np.append(y, 0), np.append(p, 1)
    return P.records(t, x, y, p)


def oracle(recs, W, H, ref_time, crf):
    src = R.Prophesee(W, H, ref_time, crf)
    return src.run(R.decode_body(recs.tobytes())), src


def run_lib(recs, W, H, ref_time, crf, splits=None, device=False):
    import torch
    pr = P.HipProphesee(W, H, ref_time, crf)
    out = [pr.start()]
    bounds = [0] + sorted(splits or []) + [len(recs)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        chunk = recs[a:b]
        if device:
            d = torch.from_numpy(chunk.view(np.uint8).copy()).to("cuda:0")
            ev = pr.push(d)
            out.append(np.frombuffer(ev.cpu().numpy().tobytes(), N.EVENT_DTYPE))
        else:
            out.append(pr.push(chunk))
    out.append(pr.finish())
    return np.concatenate(out), pr


def same(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


def test_device_exp_equals_host():
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(-500, 500, 1 << 21), rng.uniform(-1, 2, 1 << 21), rng.uniform(-750, 720, 1 << 18),
                         np.array([0.0, -0.0, 1e-300, 512.0, -512.0, 709.79, -745.2, math.inf, -math.inf])])
    assert np.array_equal(P.exp_device(xs).view(np.uint64), P.exp(xs).view(np.uint64))


@pytest.mark.parametrize("crf", [None, 0, 3, 9])
@pytest.mark.parametrize("ref_time", [1, 20])
def test_random_recordings_equal_the_oracle(crf, ref_time):
    W, H = 46, 30
    recs = recording(100 + ref_time + (crf or 0), W, H, 6000)
    want, src = oracle(recs, W, H, ref_time, crf)
    got, pr = run_lib(recs, W, H, ref_time, crf, device=True)
    assert same(got, want)
    assert np.array_equal(pr.running_intensities(), src.running_intensities())


def test_no_crf_equals_the_mirror():
    import host_py as Hst
    W, H = 46, 30
    recs = recording(7, W, H, 5000)
    dec = P.decode(recs)
    dvs = np.zeros(len(dec), Hst.DVS_DTYPE)
    for f in ("t", "x", "y", "p"):
        dvs[f] = dec[f]
    mirror, _ = Hst.prophesee(dvs, W, H, 20)  # consume() and end_events; not the start-up frames
    got, _ = run_lib(recs, W, H, 20, None)
    start = len(got) - len(mirror)
    assert start == W * H and same(got[start:], mirror)


def test_splits_give_identical_output():
    W, H = 46, 30
    recs = recording(9, W, H, 4000)
    whole, _ = run_lib(recs, W, H, 1, 3)
    rng = np.random.default_rng(4)
    for k in (1, 7, 60):
        cuts = sorted(set(rng.integers(1, len(recs), k).tolist()))
        assert same(run_lib(recs, W, H, 1, 3, cuts, device=k == 7)[0], whole)
    one_per_call = list(range(1, 300))
    assert same(run_lib(recs[:300], W, H, 1, 3, one_per_call)[0], run_lib(recs[:300], W, H, 1, 3)[0])


def test_hd_recording_equals_the_oracle():
    W, H = 1280, 720
    recs = recording(21, W, H, 1_000_000, span=2_000_000)
    want, _ = oracle(recs, W, H, 1, 3)
    got, _ = run_lib(recs, W, H, 1, 3, splits=[1 << 19], device=True)
    assert same(got, want)


def test_bad_records():
    W, H, V = 8, 4, R.VIEW_INTERVAL
    good = P.records([5, 9, 40, V + 50, V + 60], [1, 2, 3, 1, 2], [0, 1, 2, 3, 0], [1, 0, 1, 0, 1])
    # x = 9 is outside the plane: in a group that completes -> refused, nothing changes
    bad = P.records([5, 9, 40, V + 50, V + 60], [1, 9, 3, 1, 2], [0, 1, 2, 3, 0], [1, 0, 1, 0, 1])
    pr = P.HipProphesee(W, H, 1, 3)
    pr.start()
    before = pr.state()
    with pytest.raises(N.AdderHipError) as ei:
        pr.push(bad)
    assert ei.value.code == P.E_BAD_RECORD and pr.bad_index == 1 and pr.state() == before
    with pytest.raises(R.BadRecord) as eo:
        oracle(bad, W, H, 1, 3)
    assert eo.value.index == 1
    # the call changed nothing: the good stream goes through as on a fresh context
    got = [pr.push(good), pr.finish()]
    want, _ = oracle(good, W, H, 1, 3)
    assert same(np.concatenate([P.HipProphesee(W, H, 1, 3).start()] + got), want)
    # the same record in the dropped last group is never looked at
    tail = P.records([5, V + 50, V + 60, V + 61], [1, 1, 9, 2], [0, 3, 0, 1], [1, 0, 1, 1])
    want, _ = oracle(tail, W, H, 1, 3)
    assert same(run_lib(tail, W, H, 1, 3)[0], want)


def test_capacity_refusal_leaves_state_unchanged():
    W, H = 46, 30
    recs = recording(5, W, H, 3000)
    pr = P.HipProphesee(W, H, 1, 3)
    ev0 = pr.start()
    before = pr.state()
    with pytest.raises(N.AdderHipError) as ei:
        pr.push(recs, out_cap=10)
    assert ei.value.code == N.E_OUT_CAPACITY and ei.value.needed > 10 and pr.state() == before
    got = np.concatenate([ev0, pr.push(recs, out_cap=ei.value.needed), pr.finish()])
    assert same(got, oracle(recs, W, H, 1, 3)[0])


def test_undersized_device_buffer_is_refused():
    import torch
    W, H = 46, 30
    recs = recording(6, W, H, 3000)
    d = torch.from_numpy(recs.view(np.uint8).copy()).to("cuda:0")
    pr = P.HipProphesee(W, H, 1, 3)
    ev0 = pr.start()
    before = pr.state()
    small = torch.zeros(100 * 12, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(N.AdderHipError) as ei:  # out_cap defaults to the bound, the tensor holds 100 events
        pr.push(d, d_out=small)
    assert ei.value.code == N.E_OUT_CAPACITY and ei.value.needed > 100 and pr.state() == before
    assert not small.any()
    with pytest.raises(N.AdderHipError) as ei:  # an out_cap beyond the tensor is cut to it
        pr.push(d, out_cap=1 << 30, d_out=small)
    assert ei.value.code == N.E_OUT_CAPACITY and pr.state() == before and not small.any()
    with pytest.raises(ValueError):  # records must be contiguous
        pr.push(d.view(-1, 2)[:, :1])
    big = torch.empty(ei.value.needed * 3, dtype=torch.int32, device="cuda:0")  # any dtype: room counted in bytes
    ev = pr.push(d, d_out=big)
    got = np.concatenate([ev0, np.frombuffer(ev.cpu().numpy().tobytes(), N.EVENT_DTYPE), pr.finish()])
    assert same(got, oracle(recs, W, H, 1, 3)[0])


def test_end_assert_refusal():
    V = R.VIEW_INTERVAL
    recs = P.records([3 + V], [0], [0], [1])
    with pytest.raises(R.EndAssert):
        oracle(recs, 2, 1, 1, None)
    pr = P.HipProphesee(2, 1, 1, None)
    pr.start()
    pr.push(recs)
    with pytest.raises(N.AdderHipError) as ei:
        pr.finish()
    assert ei.value.code == P.E_END_ASSERT
    for call in (lambda: pr.push(recs), pr.finish):  # the reference stops there: only reset is accepted
        with pytest.raises(N.AdderHipError) as ei:
            call()
        assert ei.value.code == P.E_ORDER
    pr.reset()
    pr.start()


def test_order_rules():
    pr = P.HipProphesee(4, 4, 1, None)
    with pytest.raises(N.AdderHipError) as ei:
        pr.push(P.records([5], [0], [0], [1]))
    assert ei.value.code == P.E_ORDER
    pr.start()
    with pytest.raises(N.AdderHipError):
        pr.start()
    pr.reset()
    assert len(pr.start()) > 0


def _dat(recs, W, H):
    return b"%% Height %d\n%% Width %d\n%% Version 2\n%% end\n" % (H, W) + b"\x00\x08" + recs.tobytes()


def test_raw_and_compressed_files(tmp_path):
    from oracle import compressed_oracle as CO
    W, H = 46, 30
    recs = recording(13, W, H, 3000)
    dat = tmp_path / "in.dat"
    dat.write_bytes(_dat(recs, W, H))
    want, _ = oracle(recs, W, H, 20, 3)
    info = P.prophesee_to_adder_file(str(dat), str(tmp_path / "o.adder"), ref_time=20, crf=3, compressed=False,
                                     chunk_records=777)
    assert info["records"] == len(recs) and info["events"] == len(want)
    meta, ev = _raw(tmp_path / "o.adder")
    assert same(ev, want)
    assert [int(v) for v in meta[:7]] == [3, W, H, 1, 20 * 10 ** 6, 20, 40]
    # compressed, a small case: byte for byte against the compressed oracle fed the oracle's events
    W, H = 16, 12
    recs = recording(14, W, H, 400, span=60000)
    dat.write_bytes(_dat(recs, W, H))
    want, _ = oracle(recs, W, H, 20, 3)
    P.prophesee_to_adder_file(str(dat), str(tmp_path / "c.adder"), ref_time=20, crf=3, compressed=True,
                              chunk_records=100)
    m = P.stream_meta(W, H, 20, True)
    assert m["adu_interval"] == 10 ** 6
    co = CO.CompressedOutput(W, H, 1, tps=m["tps"], ref_interval=20, delta_t_max=m["delta_t_max"],
                             adu_interval=m["adu_interval"], source_camera=P.SOURCE_CAMERA_DVS, time_mode=1,
                             c_thresh_max=7)
    for e in want:
        co.ingest_event(int(e["x"]), int(e["y"]), int(e["c"]), int(e["d"]), int(e["t"]))
    assert (tmp_path / "c.adder").read_bytes() == co.close()


def test_round_trip_through_adder_to_dvs(tmp_path):
    from adder_amd import adder_to_dvs_file
    W, H = 46, 30
    recs = recording(17, W, H, 4000)
    dat = tmp_path / "in.dat"
    dat.write_bytes(_dat(recs, W, H))
    P.prophesee_to_adder_file(str(dat), str(tmp_path / "a.adder"), ref_time=1, crf=3, compressed=False)
    for reorder in (False, True):
        back = tmp_path / f"back{int(reorder)}.dat"
        adder_to_dvs_file(str(tmp_path / "a.adder"), str(back), reorder=reorder, date="2024-01-01 00:00:00")
        data = back.read_bytes()
        try:
            _, want = R.transcode(data, ref_time=1, crf=3)
        except R.EndAssert:  # the reference's assert: the library refuses the same file
            with pytest.raises(N.AdderHipError) as ei:
                P.prophesee_to_adder_file(str(back), str(tmp_path / "b.adder"), ref_time=1, crf=3, compressed=False)
            assert ei.value.code == P.E_END_ASSERT
        else:
            P.prophesee_to_adder_file(str(back), str(tmp_path / "b.adder"), ref_time=1, crf=3, compressed=False)
            assert same(_raw(tmp_path / "b.adder")[1], want)
        # one more record, one tick after the largest t, keeps every pixel's last t below running_t
        ts = np.frombuffer(data[R.parse_header(data)[0]:], P.RECORD_DTYPE)["t"]
        data += P.records([int(ts.max()) + 1], [0], [0], [1]).tobytes()
        back.write_bytes(data)
        src, want = R.transcode(data, ref_time=1, crf=3)
        P.prophesee_to_adder_file(str(back), str(tmp_path / "b.adder"), ref_time=1, crf=3, compressed=False)
        assert same(_raw(tmp_path / "b.adder")[1], want) and len(want) > 2 * W * H


def _raw(path):
    import host_py as Hst
    return Hst.decode_raw(path.read_bytes())


def test_c_example(tmp_path):
    import subprocess
    W, H = 46, 30
    recs = recording(19, W, H, 3000)
    dat = tmp_path / "in.dat"
    dat.write_bytes(_dat(recs, W, H))
    exe = tmp_path / "prophesee_to_adder"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    pkg = os.path.join(ROOT, "adder-codec-rs_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "examples", "prophesee_to_adder.c"), "-L", pkg, "-ladder_hip", "-L",
                           os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + pkg, "-o", str(exe)])
    subprocess.check_call([str(exe), str(dat), str(tmp_path / "c.adder"), "--ref-time", "20", "--crf", "3",
                           "--raw"])
    want, _ = oracle(recs, W, H, 20, 3)
    assert same(_raw(tmp_path / "c.adder")[1], want)
    # the tool's own format: the same bytes as the Python wrapper's compressed file
    subprocess.check_call([str(exe), str(dat), str(tmp_path / "z.adder"), "--ref-time", "20", "--crf", "5"])
    P.prophesee_to_adder_file(str(dat), str(tmp_path / "zp.adder"), ref_time=20, crf=5, compressed=True)
    assert (tmp_path / "z.adder").read_bytes() == (tmp_path / "zp.adder").read_bytes()
    r = subprocess.run([str(exe), str(dat), str(tmp_path / "d.adder"), "--features"], capture_output=True)
    assert r.returncode == 2
