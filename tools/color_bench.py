"""Measures the colour-to-gray step on the GPU and prints one JSON object:

  kernel      adder_color_to_gray_device on one packed 1080p frame and on a packed 60-frame 1080p batch: device events
              around a run of launches, the median of several runs, as us per call and as bytes moved per second
              (4 bytes per pixel: 3 read, 1 written).  One frame's 8 MB stay in the 256 MB Infinity Cache from launch to
              launch; the batch's 498 MB do not.
  batch       a one-channel 1080p context in the reference's default mode, 60 frames resident in HBM: ms per frame of
              adder_hip_integrate_device (gray frames; adder_hip_last_batch_ms, the frame kernels and their expansion)
              next to the host's wall clock around call + finish for the gray batch and for
              adder_hip_integrate_rgb_device on the colour frames (conversion included), alternating.
  mirror      the C++ mirror's consume() loop over 30 colour 1080p frames, gray transcode, default quality, with
              Framed::convert_on_device off (the CPU loop, a 2.1 MB upload per frame) and on (a 6.2 MB upload per frame,
              converted on the device), alternating; wall-clock ms per frame, the upload included on either side.

    python tools/color_bench.py [--repeats 5] [--only kernel|batch|mirror]

--only kernel is the form to run under `rocprofv3 --kernel-trace` for the kernel's own duration per dispatch.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "adder-codec-rs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H = 1920, 1080


def kernel_times(torch, A, frames, launches, repeats):
    d_rgb = torch.randint(0, 256, (frames, H, W, 3), dtype=torch.uint8, device="cuda:0")
    d_gray = torch.empty((frames, H, W), dtype=torch.uint8, device="cuda:0")
    for _ in range(3):
        A.to_gray_device(d_rgb, d_gray)
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            A.to_gray_device(d_rgb, d_gray)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1000.0 / launches)
    med = statistics.median(us)
    return {"frames": frames, "launches_per_run": launches, "us_per_call": med, "us_min": min(us), "us_max": max(us),
            "us_per_frame": med / frames, "bytes_per_second": 4.0 * W * H * frames / (med * 1e-6)}


def batch_times(torch, A, repeats, frames=60):
    d_rgb = torch.empty((frames, H, W, 3), dtype=torch.uint8, device="cuda:0")
    A.synth_clip_device(d_rgb, A.CONTENT_SCENE, W, H, 3, num_frames=frames)
    d_gray = A.to_gray_device(d_rgb).reshape(frames, -1)
    hv = A.HipVideo(W, H, 1)
    cap = W * H * frames * 5 // 4  # (events: above what a scene clip produces, below the worst case -- as bench.py sizes it)
    d_out = torch.empty(cap * 12, dtype=torch.uint8, device="cuda:0")
    d_offs = torch.zeros(frames + 1, dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    out = {"gray_ms_per_frame": [], "gray_kernels_ms_per_frame": [], "rgb_ms_per_frame": []}
    for k in range(4 + 2 * repeats):  # (the first batches warm up the context's launch plan)
        rgb = k % 2 == 1
        hv.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if rgb:
            hv.integrate_rgb_device(d_rgb, d_out, d_offs, stream=s)
        else:
            hv.integrate_device(d_gray, d_out, d_offs, stream=s)
        hv.finish()
        t1 = time.perf_counter()
        if k >= 4:
            out["rgb_ms_per_frame" if rgb else "gray_ms_per_frame"].append((t1 - t0) * 1000.0 / frames)
            if not rgb:
                out["gray_kernels_ms_per_frame"].append(hv.last_batch_ms() / frames)
    res = {k: statistics.median(v) for k, v in out.items()}
    res["frames"] = frames
    res["kernel"] = A.KERNEL_NAMES[hv.last_batch_kernel()]
    hv.close()
    return res


def mirror_times(torch, A, repeats, frames=30):
    import host_py as Hst
    L = Hst.lib()
    fn = L.adder_host_transcode_raw_ex
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_int, C.c_uint32,
                   C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_char_p, C.POINTER(C.c_uint32), C.c_int, C.c_void_p,
                   C.POINTER(C.c_double)]
    d_rgb = torch.empty((frames, H, W, 3), dtype=torch.uint8, device="cuda:0")
    A.synth_clip_device(d_rgb, A.CONTENT_SCENE, W, H, 3, num_frames=frames)
    clip = np.ascontiguousarray(d_rgb.cpu().numpy())
    ms = {0: [], 1: []}
    events = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(2 + 2 * repeats):
            on = k % 2
            secs, chunks = C.c_double(0.0), C.c_uint32(0)
            n = fn(clip.ctypes.data, frames, W, H, 3, 0, 30.0, -1, 255, 7650, 1, 1, 1, -1,
                   os.path.join(tmp, f"m{on}.adder").encode(), C.byref(chunks), on, None, C.byref(secs))
            assert n >= 0, Hst.err()
            events[on] = n
            if k >= 2:
                ms[on].append(secs.value * 1000.0 / frames)
    assert events[0] == events[1]
    return {"frames": frames, "events": events[0], "cpu_convert_ms_per_frame": statistics.median(ms[0]),
            "device_convert_ms_per_frame": statistics.median(ms[1]),
            "cpu_convert_runs": ms[0], "device_convert_runs": ms[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("kernel", "batch", "mirror"))
    args = ap.parse_args()
    import torch
    import adder_amd as A
    assert torch.cuda.is_available(), "color_bench.py measures on the GPU: no device, no numbers"
    res = {"plane": [W, H]}
    if args.only in (None, "kernel"):
        res["kernel_1_frame"] = kernel_times(torch, A, 1, 400, args.repeats)
        res["kernel_60_frames"] = kernel_times(torch, A, 60, 20, args.repeats)
    if args.only in (None, "batch"):
        res["batch"] = batch_times(torch, A, args.repeats)
    if args.only in (None, "mirror"):
        res["mirror"] = mirror_times(torch, A, args.repeats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
