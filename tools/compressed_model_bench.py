"""Measures the compressed codec's source model on the device beside the host sink, and prints one JSON
object.  One MI355X; every step runs in this one process, one after the other.

Events: a scene clip transcoded by HipVideo at the reference's default quality (crf 3: c_thresh 2, 7, 7; Collapse,
AbsoluteT, ref 255), at config 5's shape (3840x2160x3) and at 1920x1080x1; they stay in HBM.

  device   HipCompressedModel.ingest of the whole stream + close, inputs resident in HBM: one warm-up pass (code
           objects, the scratch), then the host's wall clock around each of `--repeats` passes (a pass ends in a stream
           synchronise; the three host waits inside a call are part of it) -- ms per ADU from the median pass, with
           the fastest and the slowest pass.  Beside it the device's own share of the same passes
           (HipCompressedModel.device_ms: event pairs around every stretch of device work between the calls' host
           waits -- the kernels, the sort, the scans and the device-to-device copies, without the waits).  A split by
           kernel is not taken here: run this tool with --only device under a kernel trace for it.
  host     the same events through CompressedEncoder.ingest + close (the existing sink: cubes, lists, model and coder
           on `--threads` workers) and the model's symbols through CompressedEncoder.ingest_symbols + close (coder
           only), same thread count -- ms per ADU, median of `--repeats`, and whether the two streams are equal.
  bytes    what crosses from the device in both forms: 12 bytes an event, 2 bytes a symbol word.

    python tools/compressed_model_bench.py [--shapes 3840x2160x3:8:4,1920x1080x1:60:30] [--repeats 5] [--threads 16]
                                           [--only device|host]
(a shape is WxHxC:frames:adu_interval)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "adder-codec-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

REF, DTM = 255, 7650


def transcode(torch, A, W, H, Cn, T):
    """-> (uint8 CUDA tensor of n 12-byte events, n)"""
    units = W * H * Cn
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.empty((T, units), dtype=torch.uint8, device="cuda")
    A.synth_clip_device(d_frames, A.CONTENT_SCENE, W, H, Cn, row_begin=0, rows=H, frame_begin=0, num_frames=T, stream=st)
    hv = A.HipVideo(W, H, Cn, time_mode=A.TIME_ABSOLUTE_T, multi_mode=A.MULTI_COLLAPSE, ref_time=REF, delta_t_max=DTM,
                    c_thresh_start=2, c_counter_start=0)
    hv.set_crf_parameters(7, 7)
    cap = int(units * T * 0.75) + 1024
    d_events = torch.empty(12 * cap, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv.integrate_device(d_frames, d_events, d_off, stream=st)
    n = hv.finish()
    del d_frames
    return d_events[:12 * n], n


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3840x2160x3:8:4,1920x1080x1:60:30")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--only", choices=("device", "host"))
    args = ap.parse_args()
    import torch
    import adder_amd as A
    assert torch.cuda.is_available(), "compressed_model_bench.py measures on the GPU: no device, no numbers"
    res = {"threads": args.threads, "crf": 3, "shapes": []}
    for spec in args.shapes.split(","):
        plane, T, adu = spec.split(":")
        W, H, Cn = (int(v) for v in plane.split("x"))
        T, adu = int(T), int(adu)
        d_events, n = transcode(torch, A, W, H, Cn, T)
        kw = dict(ref_interval=REF, adu_interval=adu, delta_t_max=DTM, c_thresh_max=7, tps=REF * 30)
        r = {"plane": [W, H, Cn], "frames": T, "adu_interval": adu, "events": n}

        def model_pass(keep):
            model = A.HipCompressedModel(W, H, Cn, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = model.ingest(d_events)
            dev = model.device_ms()
            first = (model.symbols_host(), model.symbol_offsets.copy()) if keep and k else None
            k2 = model.finish()
            dev += model.device_ms()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            last = (model.symbols_host(), model.symbol_offsets.copy()) if keep and k2 else None
            c = model.counters()
            model.close()
            return ms, k + k2, [x for x in (first, last) if x], c, dev

        _, adus, sym, counters, _ = model_pass(True)  # warm-up; the symbols for the host leg
        r["adus"] = adus
        words = sum(len(s) for s, _ in sym)
        kept = counters["events_in"] - counters["events_dropped"]
        r["counters"] = counters
        r["bytes_to_host"] = {"events_12B": 12 * n, "symbols_2B": 2 * words, "symbols_per_event": words / max(n, 1),
                              "reconstructed_events_stay_in_hbm": kept}
        if args.only in (None, "device"):
            passes = [model_pass(False) for _ in range(args.repeats)]
            ms = [q[0] for q in passes]
            r["device_ms_per_adu"] = {k: (v / adus if k != "runs" else v) for k, v in spread(ms).items()}
            r["device_spans_ms_per_adu"] = {k: (v / adus if k != "runs" else v)
                                            for k, v in spread([q[4] for q in passes]).items()}
            r["device_events_per_s"] = n / (statistics.median(ms) * 1e-3)
        if args.only in (None, "host"):
            ev = np.frombuffer(d_events.cpu().numpy().tobytes(), A.EVENT_DTYPE)
            enc_kw = dict(tps=REF * 30, ref_interval=REF, delta_t_max=DTM, adu_interval=adu, c_thresh_max=7,
                          threads=args.threads)
            per_adu = [s[int(o[a]):int(o[a + 1])] for s, o in sym for a in range(len(o) - 1)]
            t_ev, t_sym, same = [], [], True
            for _ in range(args.repeats):
                enc = A.CompressedEncoder(W, H, Cn, **enc_kw)
                t0 = time.perf_counter()
                enc.ingest(ev)
                a = enc.close()
                t_ev.append((time.perf_counter() - t0) * 1e3)
                enc.destroy()
                enc = A.CompressedEncoder(W, H, Cn, **enc_kw)
                t0 = time.perf_counter()
                for s in per_adu:
                    enc.ingest_symbols(s)
                b = enc.close()
                t_sym.append((time.perf_counter() - t0) * 1e3)
                enc.destroy()
                same = same and a == b
            r["host_ms_per_adu"] = {
                "ingest_events": {k: (v / adus if k != "runs" else v) for k, v in spread(t_ev).items()},
                "ingest_symbols": {k: (v / adus if k != "runs" else v) for k, v in spread(t_sym).items()}}
            r["streams_equal"], r["stream_bytes"] = same, len(a)
        res["shapes"].append(r)
        del d_events
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
