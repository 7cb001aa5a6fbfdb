"""Timing helper (not a test): time-mode migration and the adder-info fold on the device (include/adder_stream.h).
The 1080p scene clip of BASELINE configs[1] (gray, 300 frames, delta_t_max 255, crf 0) is transcoded on the device
and its events, still in HBM, are migrated DeltaT -> AbsoluteT (in one call, in place, in 60-frame batches), back
AbsoluteT -> DeltaT, and folded for the dynamic range in both time modes.  adder_dvs_convert_device on the same
stream in the same process is the yardstick.  Prints one JSON line per case (and, with OUT=<path>, writes them to that
file too): events, median and best of REPS wall times (the call returns after the device is done) and events / s.

    python tools/stream_tools_bench.py     # env: W, H, T, REPS, OUT
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "adder-codec-rs_amd"))
import torch  # noqa: E402

import adder_amd as A  # noqa: E402
from adder_amd import dvs, stream_tools as T_  # noqa: E402

E = os.environ
W, H, T = int(E.get("W", 1920)), int(E.get("H", 1080)), int(E.get("T", 300))
REPS = int(E.get("REPS", 5))
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


def timed(case, n, fn, hd):
    ts = []
    for _ in range(REPS + 1):  # the first call also allocates the scratch
        hd.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = ts[1:]
    med = statistics.median(ts)
    emit(case=case, events=n, ms_median=med * 1e3, ms_best=min(ts) * 1e3, events_per_s=n / med)


ev, offs, n = transcode()
name = f"{W}x{H} gray x {T}"
kw = dict(codec_version=2, ref_interval=255, source_camera=0)

hd = dvs.HipDvs(W, H, 1, time_mode=0, ref_interval=255, source_camera=0)
timed(f"{name}: adder_dvs_convert_device, one call (yardstick)", n, lambda: hd.convert(ev, dvs.OUT_DAT), hd)
hd.close()

fwd = T_.HipStreamMigrator(W, H, 1, time_mode=0, out_time_mode=1, **kw)
out = torch.empty_like(ev)
timed(f"{name}: migrate DeltaT -> AbsoluteT, one call", n, lambda: fwd.migrate(ev, out=out), fwd)
assert fwd.bad_index is None


def batched():
    for f0 in range(0, T, 60):
        a, b = int(offs[f0]), int(offs[min(f0 + 60, T)])
        fwd.migrate(ev[12 * a:12 * b], out=out[12 * a:12 * b])


timed(f"{name}: migrate DeltaT -> AbsoluteT, 60-frame batches", n, batched, fwd)
fwd.close()

inv = T_.HipStreamMigrator(W, H, 1, time_mode=1, out_time_mode=0, **kw)
back = torch.empty_like(ev)
timed(f"{name}: migrate AbsoluteT -> DeltaT, one call", n, lambda: inv.migrate(out, out=back), inv)
assert inv.bad_index is None
inv.close()
# Collapse mode at delta_t_max 255 holds D_EMPTY events, so forward then inverse is the identity and nothing else is
# claimed of the AbsoluteT stream in between
assert torch.equal(back, ev), "forward then inverse is not the identity"
del back

for tm, src in ((0, ev), (1, out)):
    hi = T_.HipStreamInfo(W, H, 1, time_mode=tm, **kw)
    timed(f"{name}: info fold, {'DeltaT' if tm == 0 else 'AbsoluteT'}, one call", n, lambda: hi.fold(src), hi)
    lo, hi_, cnt = hi.range()
    emit(case=f"{name}: dynamic range, {'DeltaT' if tm == 0 else 'AbsoluteT'}", min=lo, max=hi_, events=cnt)
    hi.close()

if E.get("OUT"):
    with open(E["OUT"], "w") as f:
        for kw_ in lines:
            f.write(json.dumps(kw_) + "\n")
