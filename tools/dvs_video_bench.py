"""Timing helper (not a test): the cost of the DVS event video (include/adder_dvs.h) over the plain ADDER -> DVS
conversion.  A 1080p gray scene clip is transcoded on the device in AbsoluteT; its events stay in HBM and are converted
in one call with the video off, with it on (the call then also schedules the pops and draws the fired events into the
frame ring), and with it on followed by finish and a device pop of every frame.  Per case: the median of REPS calls
after one warm-up call (which also allocates the scratch), a host clock around work that ends in a device
synchronise, reset and synchronised before every call.  Prints one JSON line per case (OUT=<path> also writes them).

    python tools/dvs_video_bench.py      # env: W, H, T, REPS, FPS, BUFFER_SECS, RING, OUT,
                                         #      PKG=<another tree's adder-codec-rs_amd, e.g. the parent commit's>

With PKG the same stream is converted by that tree's library; the video cases are left out when it has none.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = os.environ
PKG = E.get("PKG") or os.path.join(ROOT, "adder-codec-rs_amd")
sys.path.insert(0, PKG)
import torch  # noqa: E402

import adder_amd as A  # noqa: E402
from adder_amd import dvs  # noqa: E402

W, H, T = int(E.get("W", 1920)), int(E.get("H", 1080)), int(E.get("T", 120))
REPS = int(E.get("REPS", 5))
FPS, BUFFER_SECS, RING = float(E.get("FPS", 100.0)), float(E.get("BUFFER_SECS", 1.0)), int(E.get("RING", 512))
REF, TPS = 255, 7650
lines = []


def emit(**kw):
    kw["pkg"] = PKG
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def transcode():
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.empty((T, W * H), dtype=torch.uint8, device="cuda")
    A.synth_clip_device(d_frames, A.CONTENT_SCENE, W, H, 1, num_frames=T, stream=st)
    d_ev = torch.empty((int(W * H * T * 0.75) + 1024, 3), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv = A.HipVideo(W, H, 1, time_mode=A.TIME_ABSOLUTE_T, multi_mode=A.MULTI_COLLAPSE, ref_time=REF, delta_t_max=REF)
    hv.update_crf(0)
    hv.integrate_device(d_frames, d_ev, d_off, stream=st)
    n = hv.finish()
    torch.cuda.synchronize()
    return d_ev[:n].view(torch.uint8).reshape(-1), n


def timed(fn, hd):
    ms, res = [], None
    for _ in range(REPS + 1):
        hd.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[1:]  # the first call allocates the scratch and loads the kernels
    return statistics.median(ms), min(ms), max(ms), res


def main():
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    ev, n = transcode()
    name = f"{W}x{H} gray x {T} AbsoluteT"
    hd = dvs.HipDvs(W, H, 1, time_mode=A.TIME_ABSOLUTE_T, ref_interval=REF, source_camera=0)
    med, lo, hi, out = timed(lambda: hd.convert(ev, dvs.OUT_DAT), hd)
    emit(case=f"{name}, video off", events_in=n, events_out=out.numel() // 8, ms_median=med, ms_min=lo, ms_max=hi)
    hd.close()
    if not hasattr(dvs.HipDvs, "enable_video"):
        return
    hd = dvs.HipDvs(W, H, 1, time_mode=A.TIME_ABSOLUTE_T, ref_interval=REF, source_camera=0)
    hd.enable_video(TPS, FPS, BUFFER_SECS, True, RING)
    med, lo, hi, out = timed(lambda: hd.convert(ev, dvs.OUT_DAT), hd)
    emit(case=f"{name}, video on: convert", events_in=n, events_out=out.numel() // 8, ms_median=med, ms_min=lo,
         ms_max=hi, fps=FPS, buffer_secs=BUFFER_SECS, ring_frames=RING, ring_needed=hd.video_ring_needed())

    def whole():
        hd.convert(ev, dvs.OUT_DAT)
        hd.video_finish()
        return hd.video_pop(device=True)[1].shape[0]
    med, lo, hi, frames = timed(whole, hd)
    emit(case=f"{name}, video on: convert + finish + device pop", events_in=n, frames=frames, ms_median=med,
         ms_min=lo, ms_max=hi, frame_bytes=frames * W * H)
    hd.close()


main()
if E.get("OUT"):
    with open(E["OUT"], "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")
