"""Timing helper (not a test): the adder-viz player on the device (include/adder_viz_player.h).  The 1080p scene clip of
BASELINE configs[1] (gray, 300 frames, delta_t_max 255, crf 0; the stream tools/player_bench.py uses) is transcoded on
the device and its events, still in HBM, are played at the reference's rate (tps / ref_interval = 30 frames per second)
with buffer limits 60 and 2, running frames into device memory: in one call and in 60-frame batches.  The same events
through adder_framer_ingest_device (the exact framer, its pops included) and through HipPlayer (the latest-event
player, u8) are timed beside it.  Prints one JSON line per case (and, with OUT=<path>, writes them to that file too):
input events, frames, best of REPS wall times (the call returns after the device is done), input events per second.

With PROFILE=<dir> the tool starts itself once more under `rocprofv3 --kernel-trace --stats` (a fresh process, one
limit, one call, one repetition) and prints the kernel split it finds in <dir>.

With DETECT=1 the viz player's feature detection is on (adder_viz_player_detect_features): the cases are named so, and
every call also finds, files and paints the features.

    python tools/viz_player_bench.py          # env: W, H, T, REPS, LIMITS=60,2, CASES=one,batches,framer,player, RING, OUT,
                                              #      DETECT
"""
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "adder-codec-rs_amd"))
import torch  # noqa: E402

import adder_amd as A  # noqa: E402
from adder_amd import player, viz_player  # noqa: E402

E = os.environ
W, H, T = int(E.get("W", 1920)), int(E.get("H", 1080)), int(E.get("T", 300))
REPS = int(E.get("REPS", 3))
LIMITS = [int(x) for x in E.get("LIMITS", "60,2").split(",")]
CASES = E.get("CASES", "one,batches,framer,player").split(",")
TPS, REF, DTM = 7650, 255, 255
# pending frames kept: the round-up of a framed stream moves a unit one source frame ahead per EVENT, so a pixel that fires
# k times per frame runs k * T frames ahead inside one call (rings of T + 8 and 4 * T + 8 were refused for the whole clip)
RING = int(E.get("RING", 16 * T + 8))
DETECT = int(E.get("DETECT", 0))
TAG = ", detection on" if DETECT else ""
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
    hv = A.HipVideo(W, H, 1, time_mode=A.TIME_DELTA_T, multi_mode=A.MULTI_COLLAPSE, ref_time=REF, delta_t_max=DTM)
    hv.update_crf(0)
    hv.integrate_device(d_frames, d_ev, d_off, stream=st)
    n = hv.finish()
    torch.cuda.synchronize()
    return d_ev[:n].view(torch.uint8).reshape(-1), d_off.cpu().numpy(), n


def timed(fn, reset):
    best, res = 1e30, None
    for _ in range(REPS + 1):  # the first call also allocates the scratch
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, res


def kernel_split(out_dir):
    """the rocprofv3 --stats table of the child run: kernel name -> (calls, total ms)"""
    rows = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6)
    return rows


def main():
    ev, offs, n = transcode()
    fps = viz_player.reconstructed_frame_rate(TPS, REF, 0)
    for limit in LIMITS:
        hp = viz_player.HipVizPlayer(W, H, 1, tps=TPS, ref_interval=REF, delta_t_max=DTM, output_fps=fps, codec_version=2,
                                     buffer_limit=limit, ring_frames=RING, form="running")
        if DETECT:
            hp.detect_features(True)
        if "one" in CASES:
            s, k = timed(lambda: len(hp.ingest(ev, max_frames=RING)), hp.reset)
            emit(case=f"{W}x{H} gray x {T}, limit {limit}, one call{TAG}", events_in=n, frames=k, ms=s * 1e3,
                 events_per_s=n / s)
        if "batches" in CASES:
            def batched():
                m = 0
                for f0 in range(0, T, 60):
                    a, b = int(offs[f0]), int(offs[min(f0 + 60, T)])
                    m += len(hp.ingest(ev[12 * a:12 * b], max_frames=RING))
                return m
            s, k = timed(batched, hp.reset)
            emit(case=f"{W}x{H} gray x {T}, limit {limit}, 60-frame batches{TAG}", events_in=n, frames=k, ms=s * 1e3,
                 events_per_s=n / s)
        hp.close()
        torch.cuda.empty_cache()
    if "framer" in CASES:
        def framed():
            fr = A.HipFramer(W, H, 1, tps=TPS, ref_interval=REF, delta_t_max=DTM, output_fps=fps, codec_version=2,
                             ring_frames=RING)
            fr.ingest_device(ev, offs)
            k = len(fr.pop()) // (W * H)
            fr.close() if hasattr(fr, "close") else None
            return k
        s, k = timed(framed, lambda: None)
        emit(case="adder_framer_ingest_device on the same events (create, ingest, pop to the host)", events_in=n,
             frames=k, ms=s * 1e3, events_per_s=n / s)
    if "player" in CASES:
        hl = player.HipPlayer(W, H, 1, time_mode=0, ref_interval=REF, tps=TPS, source_camera=0, playback_fps=fps, out="u8")
        buf = torch.empty((RING,) + hl.shape, dtype=torch.uint8, device="cuda")
        s, k = timed(lambda: len(hl.play(ev, frames=buf)), hl.reset)
        emit(case="HipPlayer (latest event, u8) on the same events, one call", events_in=n, frames=k, ms=s * 1e3,
             events_per_s=n / s)
        hl.close()
    if E.get("PROFILE"):
        out_dir = E["PROFILE"]
        env = dict(E, REPS="0", LIMITS=str(LIMITS[0]), CASES="one")
        env.pop("PROFILE")
        env.pop("OUT", None)
        subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--",
                               sys.executable, os.path.abspath(__file__)], env=env)
        for name, (calls, ms) in sorted(kernel_split(out_dir).items(), key=lambda kv: -kv[1][1])[:16]:
            emit(kernel=name[:90], calls=calls, total_ms=ms)
    if E.get("OUT"):
        with open(E["OUT"], "w") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
