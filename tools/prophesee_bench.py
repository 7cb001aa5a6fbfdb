"""Timing helper (not a test): Prophesee .dat records -> ADDER on the device (include/adder_prophesee.h).  A seeded
1280x720 recording (30 % of the records on 5 % hot pixels, as in tools/sparse_bench.py, t spread at RATE records per
second of camera time) is pushed in calls of 2^22 records resident in HBM, AdderEvents out in HBM; one call more goes first, untimed.  Prints one JSON
line per case (and, with OUT=<path>, writes them to that file too): records, events, wall time of the pushes (each
call returns after the device is done) and camera records per second.  Cases: `hd` (the floored one), `skewed` (a
few pixels hold long runs; reported only) and `mirror` (the C++ mirror, host_py.prophesee, on the first 2^20 records).
The split between step generation and integration comes from a separate `rocprofv3 --kernel-trace --stats` run of
the `hd` case (pph_* and chain_* kernels vs adder_sparse_* kernels and the hipCUB sort / scan each side launches).

    python tools/prophesee_bench.py       # env: CALLS, RATE, CASES=hd,skewed,mirror, OUT
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

from adder_amd import prophesee as P  # noqa: E402

E = os.environ
W, H = 1280, 720
CALL = 1 << 22
CALLS = int(E.get("CALLS", 4))
RATE = float(E.get("RATE", 2e7))
CASES = E.get("CASES", "hd,skewed,mirror").split(",")
lines = []


def emit(**kw):
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def recording(n, seed, hot_px, hot_share):
    """Device records: t sorted over n / RATE seconds of camera time, pixels uniform except hot_share of the records
    on hot_px pixels."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    span = max(2, int(n / RATE * 1e6))
    t = torch.sort(torch.randint(2, 2 + span, (n,), device="cuda", generator=g, dtype=torch.int64))[0]
    px = torch.randint(0, W * H, (n,), device="cuda", generator=g, dtype=torch.int64)
    hot = torch.randperm(W * H, device="cuda", generator=g)[:hot_px]
    m = torch.rand(n, device="cuda", generator=g) < hot_share
    px[m] = hot[torch.randint(0, hot_px, (int(m.sum()),), device="cuda", generator=g)]
    p = torch.randint(0, 2, (n,), device="cuda", generator=g, dtype=torch.int64)
    data = (p << 28) | ((px // W) << 14) | (px % W)
    rec = torch.stack([t, data], 1).to(torch.int32)  # little-endian u32 t, i32 data
    return rec.contiguous().view(torch.uint8).reshape(-1)


def run(name, hot_px, hot_share):
    n = CALL * CALLS
    rec = recording(n + CALL, 5, hot_px, hot_share)  # the first call warms up (allocations) and is not timed
    pr = P.HipProphesee(W, H, 1, 3)
    pr.start()
    cap = 2 * (CALL + (1 << 21)) * pr.events_per_step
    d_out = torch.empty(cap * 12, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    events, secs = 0, 0.0
    for k in range(CALLS + 1):
        chunk = rec[k * CALL * 8:(k + 1) * CALL * 8]
        t0 = time.perf_counter()
        ev = pr.push(chunk, out_cap=cap, d_out=d_out)
        if k:
            secs += time.perf_counter() - t0
            events += ev.numel() // 12
    end = len(pr.finish())
    pr.close()
    emit(case=name, width=W, height=H, records=n, calls=CALLS, events=events, end_events=end,
         push_seconds=round(secs, 4), records_per_s=round(n / secs), floor=2e8 if name == "hd" else None)
    return rec


def main():
    rec = None
    if "hd" in CASES:
        rec = run("hd", int(W * H * 0.05), 0.3)
    if "skewed" in CASES:
        run("skewed", 16, 0.5)
    if "mirror" in CASES:
        import host_py as Hst
        if rec is None:
            rec = recording(CALL, 5, int(W * H * 0.05), 0.3)
        r = np.frombuffer(rec[: 8 << 20].cpu().numpy().tobytes(), P.RECORD_DTYPE)
        dec = P.decode(r)
        dvs = np.zeros(len(dec), Hst.DVS_DTYPE)
        for f in ("t", "x", "y", "p"):
            dvs[f] = dec[f]
        t0 = time.perf_counter()
        ev, calls = Hst.prophesee(dvs, W, H, 1)
        s = time.perf_counter() - t0
        emit(case="mirror", records=len(dvs), events=len(ev), seconds=round(s, 3), records_per_s=round(len(dvs) / s),
             note="C++ mirror: start-up, consume() per group, end_events")
    if E.get("OUT"):
        with open(E["OUT"], "w") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
