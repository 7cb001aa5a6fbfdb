"""Timing helper (not a test): ADDER -> DVS on the device (include/adder_dvs.h).  The 1080p scene clip of BASELINE
configs[1] (gray, 300 frames, delta_t_max 255, crf 0) is transcoded on the device and its events, still in HBM, are
converted to .dat records: in one call, in 60-frame batches, with --reorder (the stable sort by t after the
conversion), and the same for configs[2] (RGB).  The CPU restatement's rate (tests/dvs_oracle.py) on a slice is there
for comparison.  Prints one JSON line per case (and, with OUT=<path>, writes them to that file too): input events,
output events, best of REPS wall times (the call returns after the device is done) and input events per second.

    python tools/dvs_bench.py            # env: W, H, T, REPS, CASES=gray,batches,reorder,rgb,cpu, OUT
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "adder-codec-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import adder_amd as A  # noqa: E402
from adder_amd import dvs  # noqa: E402

E = os.environ
W, H, T = int(E.get("W", 1920)), int(E.get("H", 1080)), int(E.get("T", 300))
REPS = int(E.get("REPS", 3))
CASES = E.get("CASES", "gray,batches,reorder,rgb,cpu").split(",")
lines = []


def emit(**kw):
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def transcode(C):
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.empty((T, W * H * C), dtype=torch.uint8, device="cuda")
    A.synth_clip_device(d_frames, A.CONTENT_SCENE, W, H, C, num_frames=T, stream=st)
    d_ev = torch.empty((int(W * H * C * T * 0.75) + 1024, 3), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv = A.HipVideo(W, H, C, time_mode=A.TIME_DELTA_T, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=255)
    hv.update_crf(0)
    hv.integrate_device(d_frames, d_ev, d_off, stream=st)
    n = hv.finish()
    torch.cuda.synchronize()
    return d_ev[:n].view(torch.uint8).reshape(-1), d_off.cpu().numpy(), n


def timed(fn, hd):
    best = 1e30
    res = None
    for _ in range(REPS + 1):  # the first call also allocates the scratch
        hd.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, res


def run_config(C, name):
    ev, offs, n = transcode(C)
    hd = dvs.HipDvs(W, H, C, time_mode=0, ref_interval=255, source_camera=0)
    if "gray" in CASES or C == 3:
        s, out = timed(lambda: hd.convert(ev, dvs.OUT_DAT), hd)
        emit(case=f"{name} one batch", events_in=n, events_out=out.numel() // 8, ms=s * 1e3, events_per_s=n / s,
             wire_bytes_in=n * (9 if C == 1 else 11))
    if "batches" in CASES and C == 1:
        def batched():
            m = 0
            for f0 in range(0, T, 60):
                a, b = int(offs[f0]), int(offs[min(f0 + 60, T)])
                m += hd.convert(ev[12 * a:12 * b], dvs.OUT_DAT).numel() // 8
            return m
        s, m = timed(batched, hd)
        emit(case=f"{name} 60-frame batches", events_in=n, events_out=m, ms=s * 1e3, events_per_s=n / s)
    if "reorder" in CASES and C == 1:
        def reordered():
            out = hd.convert(ev, dvs.OUT_DAT)
            hd.sort(out, dvs.OUT_DAT)
            return out
        s, out = timed(reordered, hd)
        emit(case=f"{name} one batch + reorder", events_in=n, events_out=out.numel() // 8, ms=s * 1e3,
             events_per_s=n / s)
    if "cpu" in CASES and C == 1:
        import dvs_oracle as R
        k = min(n, 300_000)
        host = np.frombuffer(ev[: 12 * k].cpu().numpy().tobytes(), A.EVENT_DTYPE)
        t0 = time.perf_counter()
        out, _ = R.DvsRestatement(W, H, 1, 0, 255, 0).run(host)
        s = time.perf_counter() - t0
        emit(case="CPU restatement (Python, one core), first events of the gray stream", events_in=k,
             events_out=len(out), ms=s * 1e3, events_per_s=k / s)
    hd.close()
    del ev
    torch.cuda.empty_cache()


if any(c in CASES for c in ("gray", "batches", "reorder", "cpu")):
    run_config(1, f"{W}x{H} gray x {T}")
if "rgb" in CASES:
    run_config(3, f"{W}x{H} RGB x {T}")
if E.get("OUT"):
    with open(E["OUT"], "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")
