"""Timing helper (not a test): the latest-event player on the device (include/adder_player.h).  The 1080p scene clip
of BASELINE configs[1] (gray, 300 frames, delta_t_max 255, crf 0; the stream tools/dvs_bench.py uses) is transcoded on
the device and its events, still in HBM, are played at 60 fps (tps 7650: FL = 127) into a preallocated frame buffer:
in one call and in 60-frame batches, f64 and u8 frames.  adder-to-dvs on the same events is timed beside it.  Prints
one JSON line per case (and, with OUT=<path>, writes them to that file too): input events, frames, best of REPS wall
times (the call returns after the device is done), input events per second and output bytes per second.

    python tools/player_bench.py            # env: W, H, T, REPS, CASES=f64,u8,batches,dvs, OUT
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "adder-codec-rs_amd"))
import torch  # noqa: E402

import adder_amd as A  # noqa: E402
from adder_amd import dvs, player  # noqa: E402

E = os.environ
W, H, T = int(E.get("W", 1920)), int(E.get("H", 1080)), int(E.get("T", 300))
REPS = int(E.get("REPS", 3))
CASES = E.get("CASES", "f64,u8,batches,dvs").split(",")
FPS, TPS = 60.0, 7650
lines = []


def emit(**kw):
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def transcode():
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.empty((T, W * H), dtype=torch.uint8, device="cuda")
    A.synth_clip_device(d_frames, A.CONTENT_SCENE, W, H, 1, num_frames=T, stream=st)
    d_ev = torch.empty((int(W * H * T * 0.75) + 1024, 3), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv = A.HipVideo(W, H, 1, time_mode=A.TIME_DELTA_T, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=255)
    hv.update_crf(0)
    hv.integrate_device(d_frames, d_ev, d_off, stream=st)
    n = hv.finish()
    torch.cuda.synchronize()
    return d_ev[:n].view(torch.uint8).reshape(-1), d_off.cpu().numpy(), n


def timed(fn, h):
    best, res = 1e30, None
    for _ in range(REPS + 1):  # the first call also allocates the scratch
        h.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, res


ev, offs, n = transcode()
for out in ("f64", "u8"):
    if out not in CASES:
        continue
    hp = player.HipPlayer(W, H, 1, time_mode=0, ref_interval=255, tps=TPS, source_camera=0, playback_fps=FPS, out=out)
    try:  # a call without room changes nothing and says how many frames the stream shows
        max_frames = len(hp.play(ev, max_frames=0))
    except A.AdderHipError as e:
        if e.code != A.E_OUT_CAPACITY:
            raise
        max_frames = e.needed
    buf = torch.empty((max_frames + 1,) + hp.shape, dtype=getattr(torch, hp.dtype.name), device="cuda")
    fb = hp.units * hp.dtype.itemsize
    s, k = timed(lambda: len(hp.play(ev, frames=buf)), hp)
    emit(case=f"{W}x{H} gray x {T}, one call, {out}", events_in=n, frames=k, ms=s * 1e3, events_per_s=n / s,
         out_bytes_per_s=k * fb / s)
    if "batches" in CASES:
        def batched():
            m = 0
            for f0 in range(0, T, 60):
                a, b = int(offs[f0]), int(offs[min(f0 + 60, T)])
                m += len(hp.play(ev[12 * a:12 * b], frames=buf))
            return m
        s, k = timed(batched, hp)
        emit(case=f"{W}x{H} gray x {T}, 60-frame batches, {out}", events_in=n, frames=k, ms=s * 1e3,
             events_per_s=n / s, out_bytes_per_s=k * fb / s)
    hp.close()
    del buf
    torch.cuda.empty_cache()
if "dvs" in CASES:
    hd = dvs.HipDvs(W, H, 1, time_mode=0, ref_interval=255, source_camera=0)
    s, o = timed(lambda: hd.convert(ev, dvs.OUT_DAT), hd)
    emit(case=f"adder-to-dvs on the same events, one call", events_in=n, events_out=o.numel() // 8, ms=s * 1e3,
         events_per_s=n / s)
    hd.close()
if E.get("OUT"):
    with open(E["OUT"], "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")
