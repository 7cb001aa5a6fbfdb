"""Measures the DAVIS -> ADDER chain on the GPU and prints one JSON object.

Seeded packets (a frame, the contrast threshold, 2^19 `before` and 2^19 `after` DVS events: 2^20 camera events per
packet, 60 % of them on 25 hot pixels as in the mirror's test) at 346x260 (DAVIS346) and at 1280x720, RawDavis mode,
tps 10^6, ref_time 5000, delta_t_max 500000, crf 2.

  device      adder_davis_push_device with the frame and both event lists resident in HBM: one warm-up push, then the
              host's wall clock around each further push (the call ends in a stream synchronise) -- us per packet, the
              median over the timed packets, and camera events per second (2^20 / that).
  mirror      the C++ mirror's Davis with chain_on_device off (the per-pixel chain on one CPU thread, 16-byte steps
              uploaded: the path the library had before the device chain) over the same packets through
              adder_host_davis.  The call also creates the context and flushes at the end, so the packet time is
              (wall clock of P packets - wall clock of 1 packet) / (P - 1).
  equal       whether the device chain's events over all packets and the finish equal the mirror's, byte for byte.

    python tools/davis_bench.py [--sizes 346x260,1280x720] [--packets 5] [--events 1048576] [--only device|mirror]

--only device is the form to run under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "adder-codec-rs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TPS, REF, DTM, CRF, MODE = 1_000_000, 5000, 500_000, 2, 1
EVENT_DTYPE = np.dtype([("t", "<i8"), ("x", "<u2"), ("y", "<u2"), ("on", "u1"), ("pad", "u1", (3,))])


def make_packets(W, H, P, n_events, seed=7):
    rng = np.random.default_rng(seed)
    packets, t = [], 40_000
    base = rng.random((H, W))
    half = n_events // 2

    def evs(lo, hi, n):
        ev = np.zeros(n, EVENT_DTYPE)
        ev["t"] = np.sort(rng.integers(lo, hi, n))
        hot = rng.integers(0, W * H, 25)
        pix = np.where(rng.random(n) < 0.6, hot[rng.integers(0, 25, n)], rng.integers(0, W * H, n))
        ev["x"], ev["y"], ev["on"] = pix % W, pix // W, rng.integers(0, 2, n)
        return ev
    for _ in range(P):
        start, end = t, t + int(rng.integers(3000, 9000))
        nxt = end + int(rng.integers(10_000, 30_000))
        frame = np.clip(base + rng.normal(0, 0.08, (H, W)), -0.05, 1.1)
        packets.append({"frame": frame, "c": 0.1 + 0.05 * rng.random(), "start": start, "end": end,
                        "before": evs(start - 25_000, start + 2000, half), "after": evs(end - 2000, nxt + 1000, n_events - half)})
        t = nxt
    return packets


def device_run(torch, D, packets, W, H):
    dv = D.HipDavis(W, H, MODE, TPS, REF, DTM, CRF)
    dev = [(torch.from_numpy(np.ascontiguousarray(p["frame"])).cuda(),
            torch.from_numpy(p["before"].view(np.uint8).reshape(-1).copy()).cuda(),
            torch.from_numpy(p["after"].view(np.uint8).reshape(-1).copy()).cuda()) for p in packets]
    cap = max(dv.push_capacity(len(p["before"]) + len(p["after"])) for p in packets)
    d_out = torch.empty(cap * 12, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    us, events, chunks = [], 0, []
    for k, (p, (f, b, a)) in enumerate(zip(packets, dev)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = dv.push(f, float(p["c"]), int(p["start"]), int(p["end"]), b, a, stream=s, d_out=d_out)
        t1 = time.perf_counter()
        if k >= 1:  # the first push warms up: code objects, scratch, the sort's temporary storage
            us.append((t1 - t0) * 1e6)
        events += out.numel() // 12
        chunks.append(out.cpu().numpy().tobytes())
    fin = dv.finish()
    chunks.append(fin.tobytes())
    dv.close()
    med = statistics.median(us)
    n_cam = len(packets[0]["before"]) + len(packets[0]["after"])
    return {"us_per_packet": med, "us_min": min(us), "us_max": max(us), "timed_packets": len(us),
            "camera_events_per_second": n_cam / (med * 1e-6), "adder_events": events + len(fin)}, b"".join(chunks)


def mirror_run(packets, W, H):
    import host_py as Hst
    kw = dict(tps=TPS, ref_time=REF, delta_t_max=DTM, crf=CRF)
    Hst.davis(packets[:1], W, H, MODE, **kw)  # warm-up: the library, the context's code objects
    t0 = time.perf_counter()
    Hst.davis(packets[:1], W, H, MODE, **kw)
    t1 = time.perf_counter()
    ev, _ = Hst.davis(packets, W, H, MODE, **kw)
    t2 = time.perf_counter()
    per = ((t2 - t1) - (t1 - t0)) / (len(packets) - 1)
    n_cam = len(packets[0]["before"]) + len(packets[0]["after"])
    return {"us_per_packet": per * 1e6, "one_packet_call_us": (t1 - t0) * 1e6, "all_packets_call_us": (t2 - t1) * 1e6,
            "camera_events_per_second": n_cam / per, "adder_events": len(ev)}, ev.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="346x260,1280x720")
    ap.add_argument("--packets", type=int, default=5)
    ap.add_argument("--events", type=int, default=1 << 20)
    ap.add_argument("--only", choices=("device", "mirror"))
    ap.add_argument("--dry-run", action="store_true", help="build the packets and stop (no GPU needed)")
    args = ap.parse_args()
    assert args.packets >= 2
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    if args.dry_run:
        for W, H in sizes:
            pk = make_packets(W, H, args.packets, args.events)
            print(json.dumps({"plane": [W, H], "packets": len(pk), "before": len(pk[0]["before"]), "after": len(pk[0]["after"])}))
        return
    import torch
    from adder_amd import davis as D
    assert torch.cuda.is_available(), "davis_bench.py measures on the GPU: no device, no numbers"
    res = {"mode": "RawDavis", "events_per_packet": args.events, "packets": args.packets, "planes": []}
    for W, H in sizes:
        packets = make_packets(W, H, args.packets, args.events)
        r = {"plane": [W, H]}
        dev_bytes = mir_bytes = None
        if args.only in (None, "device"):
            r["device"], dev_bytes = device_run(torch, D, packets, W, H)
        if args.only in (None, "mirror"):
            r["mirror"], mir_bytes = mirror_run(packets, W, H)
        if dev_bytes is not None and mir_bytes is not None:
            r["equal"] = dev_bytes == mir_bytes
            r["speedup"] = r["mirror"]["us_per_packet"] / r["device"]["us_per_packet"]
        res["planes"].append(r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
