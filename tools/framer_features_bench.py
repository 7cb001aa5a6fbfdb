"""Timing helper (not a test): feature detection while framing (adder_framer_detect_features).

The 1080p scene clip (gray, T frames, delta_t_max 255, crf 0) is transcoded on the device as DeltaT and as AbsoluteT v2;
with the events resident in HBM, adder_framer_ingest_device takes the whole stream in one call with detection off and
with detection on, in the same process, and adder_dvs_convert_device on the same stream is the yardstick.  A call's
wall time includes its final wait; median and the five values of REPS repetitions after a warm-up, each on a fresh
context whose buffers exist before the clock starts (adder_framer_reserve_features).  One JSON line per case.

Every GPU step is a child process under its own `timeout -k 10`; after a step that fails nothing more is started.

    python tools/framer_features_bench.py                 # all steps; env: W, H, T, REPS, OUT (a file that collects the lines)
    python tools/framer_features_bench.py --step delta    # one step in this process: delta | absolute
    python tools/framer_features_bench.py --off-only      # the detection-off cases alone (runs on a tree without detection)
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.environ.get("ADDER_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = os.environ
W, H, T = int(E.get("W", 1920)), int(E.get("H", 1080)), int(E.get("T", 300))
REPS = int(E.get("REPS", 5))
STEP_TIMEOUT = int(E.get("STEP_TIMEOUT", 420))


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if E.get("OUT"):
        with open(E["OUT"], "a") as f:
            f.write(line + "\n")


def step(time_mode_name, off_only):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "adder-codec-rs_amd"))
    import torch
    import adder_amd as A
    from adder_amd import dvs

    tm = A.TIME_DELTA_T if time_mode_name == "delta" else A.TIME_ABSOLUTE_T
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.empty((T, W * H), dtype=torch.uint8, device="cuda")
    A.synth_clip_device(d_frames, A.CONTENT_SCENE, W, H, 1, num_frames=T, stream=st)
    d_ev = torch.empty((int(W * H * T * 0.75) + 1024, 3), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv = A.HipVideo(W, H, 1, time_mode=tm, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=255)
    hv.update_crf(0)
    hv.integrate_device(d_frames, d_ev, d_off, stream=st)
    n = hv.finish()
    torch.cuda.synchronize()
    del d_frames, hv
    ev = d_ev[:n]
    offs = [0, n]
    name = f"{W}x{H} gray x {T}, {'DeltaT' if tm == A.TIME_DELTA_T else 'AbsoluteT v2'}, crf 0"

    def framer(detect):
        # the whole stream goes in without a pop: the ring holds all its frames
        fr = A.HipFramer(W, H, 1, tps=255 * 30, ref_interval=255, delta_t_max=255, output_fps=30.0, codec_version=2,
                         time_mode=tm, source_camera=A.FRAMED_U8, ring_frames=T + 120)
        if detect:
            fr.detect_features(True)
            fr.reserve_features(n)
        return fr

    def timed(case, detect):
        ts, count = [], None
        for _ in range(REPS + 1):
            fr = framer(detect)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fr.ingest_device(ev, offs, stream=st)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            try:
                ready = fr.frames_ready()
            except A.AdderHipError as e:  # e.g. the frame ring too small for a clock that ran away: reported, not hidden
                ready = str(e)
            if detect:
                count = len(fr.features())
            fr.close()
        ts = ts[1:]
        med = statistics.median(ts)
        emit(case=f"{name}: ingest_device, detection {'on' if detect else 'off'}", events=n, ms=[round(t * 1e3, 3) for t in ts],
             ms_median=med * 1e3, events_per_s=n / med, frames_ready=ready, features=count)
        return med

    off = timed("off", False)
    if off_only:
        return
    on = timed("on", True)
    if tm == A.TIME_DELTA_T:
        hd = dvs.HipDvs(W, H, 1, time_mode=0, ref_interval=255, source_camera=0)
    else:
        hd = dvs.HipDvs(W, H, 1, time_mode=1, ref_interval=255, source_camera=0)
    evb = ev.view(torch.uint8).reshape(-1)
    ts = []
    for _ in range(REPS + 1):
        hd.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hd.convert(evb, dvs.OUT_DAT)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = ts[1:]
    y = statistics.median(ts)
    emit(case=f"{name}: adder_dvs_convert_device (yardstick)", events=n, ms=[round(t * 1e3, 3) for t in ts],
         ms_median=y * 1e3, events_per_s=n / y)
    emit(case=f"{name}: ratios", on_over_off=on / off, on_over_dvs=on / y, on_over_dvs_plus_off=on / (y + off))


def main():
    args = sys.argv[1:]
    off_only = "--off-only" in args
    if "--step" in args:
        step(args[args.index("--step") + 1], off_only)
        return 0
    for name in ("delta", "absolute"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--step", name]
        if off_only:
            cmd.append("--off-only")
        rc = subprocess.call(cmd)
        if rc != 0:  # a fault, an abort or a time limit: nothing more is started on the device
            print(f"step {name} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
