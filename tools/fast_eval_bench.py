"""Measures adder_fast_evaluate_device on the GPU beside the same logic header on the CPUs, and prints one
JSON object.

Seeded frames (mild noise under bright squares, shifted from frame to frame) and a prediction plane with about one
position in a hundred set, at 346x260, 1280x720 and 1920x1080, one channel, threshold 30, without and with
suppression.

  device   HipFastEval.evaluate_device on `--frames` frames (60) with frames and predictions resident in HBM: one
           warm-up call (code objects, the scratch), then the host's wall clock around each of `--calls` further calls
           (a call ends in a stream synchronise) -- us per frame from the median call.
  host     csrc/adder_fast_logic.hpp as g++ -O3 builds it (tests/cpu_sim/fast_eval_sim.cpp: fes_evaluate), the frames
           spread over `--threads` threads (default: the CPUs this process may use, 16 at most) -- us per frame of the
           whole batch's wall clock.
  equal    whether both give the same counts for every frame.
  bytes    what a frame's evaluation moves at least: the frame read, the mask written and read back, the prediction read
           (4 B per pixel); with suppression also the score plane written and read (6 B per pixel) -- and the GB/s
           that is at the device's time.

    python tools/fast_eval_bench.py [--sizes 346x260,1280x720,1920x1080] [--frames 60] [--calls 5] [--only device|host]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "adder-codec-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

THRESHOLD = 30


def make_inputs(W, H, n, seed=11):
    rng = np.random.default_rng(seed)
    base = rng.integers(60, 140, (H, W)).astype(np.uint8)
    for _ in range(max(4, W * H // 4000)):
        s = int(rng.integers(5, 24))
        x, y = int(rng.integers(0, max(W - s, 1))), int(rng.integers(0, max(H - s, 1)))
        base[y:y + s, x:x + s] = int(rng.integers(180, 256))
    frames = np.stack([np.roll(base, (k, 2 * k), axis=(0, 1)) for k in range(n)])
    pred = (rng.integers(0, 100, (n, H, W)) == 0).astype(np.uint8)
    return frames, pred


def device_run(torch, A, frames, pred, nonmax, calls):
    n, H, W = frames.shape
    fe = A.HipFastEval(W, H, 1, threshold=THRESHOLD, nonmax=nonmax)
    d_frames, d_pred = torch.from_numpy(frames).cuda(), torch.from_numpy(pred).cuda()
    s = torch.cuda.current_stream().cuda_stream
    res = fe.evaluate_device(d_frames, d_pred, stream=s)  # warm-up
    us = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fe.evaluate_device(d_frames, d_pred, stream=s)
        us.append((time.perf_counter() - t0) * 1e6)
    fe.close()
    med = statistics.median(us)
    per_pixel = 6 if nonmax else 4
    moved = per_pixel * W * H
    return {"us_per_frame": med / n, "us_per_call_min": min(us), "us_per_call_max": max(us), "timed_calls": calls,
            "bytes_per_frame": moved, "bytes_per_pixel": per_pixel, "gb_per_s": moved / (med / n * 1e-6) / 1e9,
            "kept_per_frame": sum(r["gt_count"] for r in res) / n}, [(r["tp"], r["fp"], r["tn"], r["fn"]) for r in res]


def host_lib(tmp):
    src = os.path.join(ROOT, "tests", "cpu_sim", "fast_eval_sim.cpp")
    lib = os.path.join(tmp, "libfast_eval_host.so")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "adder-codec-rs_amd", "csrc"), src, "-o", lib])
    L = C.CDLL(lib)
    L.fes_evaluate.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p]
    return L


def host_run(L, frames, pred, nonmax, threads):
    n, H, W = frames.shape
    out, ratios = np.zeros((n, 5), np.uint64), np.zeros((n, 3), np.float64)

    def one(k):
        work = np.empty(2 * W * H, np.uint8)
        L.fes_evaluate(frames[k].ctypes.data, W, H, 1, THRESHOLD, int(nonmax), pred[k].ctypes.data, work.ctypes.data,
                       out[k].ctypes.data, ratios[k].ctypes.data)
    one(0)  # warm-up: the library's pages
    with ThreadPoolExecutor(threads) as pool:
        t0 = time.perf_counter()
        list(pool.map(one, range(n)))
        t1 = time.perf_counter()
    return {"us_per_frame": (t1 - t0) * 1e6 / n, "threads": threads}, [tuple(int(v) for v in r[:4]) for r in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="346x260,1280x720,1920x1080")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--only", choices=("device", "host"))
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    res = {"threshold": THRESHOLD, "frames_per_call": args.frames, "planes": []}
    with tempfile.TemporaryDirectory() as tmp:
        L = host_lib(tmp) if args.only in (None, "host") else None
        if args.only in (None, "device"):
            import torch
            import adder_amd as A
            assert torch.cuda.is_available(), "fast_eval_bench.py measures on the GPU: no device, no numbers"
        for W, H in sizes:
            frames, pred = make_inputs(W, H, args.frames)
            for nonmax in (False, True):
                r = {"plane": [W, H], "nonmax": nonmax}
                dev = host = None
                if args.only in (None, "device"):
                    r["device"], dev = device_run(torch, A, frames, pred, nonmax, args.calls)
                if L is not None:
                    r["host"], host = host_run(L, frames, pred, nonmax, args.threads)
                if dev is not None and host is not None:
                    r["equal"] = dev == host
                    r["speedup"] = r["host"]["us_per_frame"] / r["device"]["us_per_frame"]
                res["planes"].append(r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
