"""Timing helper (not a test): the quality metrics on the device (include/adder_quality.h).  Prints one JSON line per
case (and, with OUT=<path>, writes them to that file too): frames, best of REPS wall times of one call (it returns after
the device is done and the results are on the host), microseconds per frame, and the bytes of the memory floor
(both inputs read once, the map written once) with their time at the measured 6.29 TB/s copy rate.

    gray     1080p gray x 60 frames: MSE+PSNR, then +SSIM, then +SSIM with the per-window map
    rgb      3840x2160 RGB x 8 frames (BASELINE config 5's shape), all three metrics
    viewer   the viewer's loop: a 1-frame transcode, the running plane copied on the device, its metrics, per frame
    cpu      the vectorised CPU restatement (tests/quality_oracle.py) of one 1080p gray frame, for scale

    python tools/quality_bench.py            # env: REPS, CASES=gray,rgb,viewer,cpu, OUT
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

E = os.environ
REPS = int(E.get("REPS", 5))
CASES = E.get("CASES", "gray,rgb,viewer,cpu").split(",")
COPY_RATE = 6.29e12
lines = []


def emit(**kw):
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def pair(W, H, C, T, seed):
    st = torch.cuda.current_stream().cuda_stream
    d_a = torch.empty((T, H, W, C), dtype=torch.uint8, device="cuda")
    A.synth_clip_device(d_a, A.CONTENT_SCENE, W, H, C, num_frames=T, stream=st)
    g = torch.Generator(device="cuda").manual_seed(seed)
    noise = torch.randint(-6, 7, d_a.shape, generator=g, device="cuda", dtype=torch.int16)
    d_b = (d_a.to(torch.int16) + noise).clamp(0, 255).to(torch.uint8)
    torch.cuda.synchronize()
    return d_a, d_b


def timed(fn):
    best, res = 1e30, None
    for _ in range(REPS + 1):  # the first call also allocates the scratch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        best = min(best, time.perf_counter() - t0)
    return best, res


def case(name, W, H, C, T, ssim, with_map, seed=1):
    d_a, d_b = pair(W, H, C, T, seed)
    q = A.HipQuality(W, H, C, ssim=ssim)
    m = torch.empty(q.map_shape(T), dtype=torch.float64, device="cuda") if with_map else None
    best, res = timed(lambda: q.compute_device(d_a, d_b, ssim_map=m))
    floor = 2 * W * H * C * T + (m.numel() * 8 if with_map else 0)
    emit(case=name, width=W, height=H, channels=C, frames=T, ssim=ssim, map=with_map, wall_ms=best * 1e3,
         us_per_frame=best * 1e6 / T, floor_bytes=floor, floor_us_per_frame=floor / COPY_RATE * 1e6 / T,
         mean_psnr=float(np.mean([r["psnr"] for r in res])),
         mean_ssim=float(np.mean([r["ssim"] for r in res])) if ssim else None)


if "gray" in CASES:
    case("1080p_gray_mse_psnr", 1920, 1080, 1, 60, False, False)
    case("1080p_gray_ssim", 1920, 1080, 1, 60, True, False)
    case("1080p_gray_ssim_map", 1920, 1080, 1, 60, True, True)
if "rgb" in CASES:
    case("4k_rgb_ssim", 3840, 2160, 3, 8, True, False)

if "viewer" in CASES:
    W, H, T = 1920, 1080, 30
    st = torch.cuda.Stream()
    d_clip = torch.empty((T, W * H), dtype=torch.uint8, device="cuda")
    A.synth_clip_device(d_clip, A.CONTENT_SCENE, W, H, 1, num_frames=T, stream=torch.cuda.current_stream().cuda_stream)
    hv = A.HipVideo(W, H, 1, time_mode=A.TIME_ABSOLUTE_T, multi_mode=A.MULTI_COLLAPSE, delta_t_max=7650,
                    c_thresh_start=2, c_counter_start=0, max_depth=20)
    hv.set_crf_parameters(7, 7)
    hv.enable_running_intensities(True)
    q = A.HipQuality(W, H, 1, ssim=True)
    d_ev = torch.empty((hv.max_events_per_frame + 1024, 3), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_plane = torch.empty((H, W, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def step(k):
        hv.integrate_device(d_clip[k:k + 1], d_ev, d_off, stream=st.cuda_stream)
        hv.running_intensities_device(d_plane, stream=st.cuda_stream)
        r = q.compute_device(d_clip[k].view(H, W, 1), d_plane, stream=st)[0]
        hv.finish()
        return r

    for k in range(5):
        step(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = [step(k) for k in range(5, T)]
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    for k in range(5, T):
        hv.integrate_device(d_clip[k:k + 1], d_ev, d_off, stream=st.cuda_stream)
        hv.finish()
    dt0 = time.perf_counter() - t0
    emit(case="viewer_loop_1080p_gray", frames=T - 5, us_per_frame=dt * 1e6 / (T - 5),
         transcode_only_us_per_frame=dt0 * 1e6 / (T - 5), mean_psnr=float(np.mean([r["psnr"] for r in res])),
         mean_ssim=float(np.mean([r["ssim"] for r in res])))

if "cpu" in CASES:
    import quality_oracle as Q
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (1080, 1920), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    t0 = time.perf_counter()
    Q.fast_ssim(a, b, want_map=False)
    emit(case="cpu_vectorised_1080p_gray_ssim", frames=1, us_per_frame=(time.perf_counter() - t0) * 1e6)

if E.get("OUT"):
    with open(E["OUT"], "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")
