"""The streams the compressed source model is checked on (tests/test_compressed_model_cpu.py against the host sink,
tests/test_gpu_compressed_model.py on the device): the reference's three stream.rs scenarios, the seeded random streams
of tests/test_compressed_product.py, the VIRAT sample, and streams built by hand for the arms the seeds
do not reach (the census in the CPU test counts every arm).  A case is a dict: name, w, h, c, tps, ref, dtm, adu, cmax,
header, events (a function -> EVENT_DTYPE array, so that importing this file costs nothing)."""
import os
import struct
import subprocess

import numpy as np

import adder_amd as A

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM_SRC = os.path.join(HERE, "cpu_sim", "compressed_model_main.cpp")


def events_of(rows):
    ev = np.zeros(len(rows), A.EVENT_DTYPE)
    for i, (x, y, c, d, t) in enumerate(rows):
        ev[i] = (x, y, c, d, 0, t)
    return ev


# ---------------------------------------------------------------- stream.rs:510-946 (bare CompressedOutput)
def _stream_rs_1():
    rows, counter = [], 0
    for _ in range(10):
        for y in range(30):
            for x in range(16):
                rows.append((x, y, 0xFF, 7, 280 + counter))
                counter += 1
    return events_of(rows)


def _stream_rs_2():
    rows, counter = [], 0
    for i in range(60):
        rows.append((12, 7, 0xFF, 7, 280 + i * 100 + counter))
        counter += 1
    rows.append((19, 14, 0xFF, 7, 280))
    for i in range(60, 70):
        rows.append((12, 7, 0xFF, 7, 280 + i * 100 + counter))
        counter += 1
    return events_of(rows)


def _stream_rs_3():
    rows, counter = [], 0
    for rep in range(2):
        for i in range(10):
            for y in range(30):
                for x in range(30):
                    if not (y == 14 and x == 14 or i % 3 == 0 and y >= 16 and x < 16):
                        rows.append((x, y, 0xFF, 7, 280 + counter))
                        counter += 1
        if rep == 0:
            rows.append((14, 14, 0xFF, 7, 280))
    return events_of(rows)


# ---------------------------------------------------------------- seeded random streams
def random_stream(w, h, channels, n, seed, d_values=(0, 1, 3, 5, 7, 8, 9, 12, 128, 200, 255)):
    """Mostly increasing time with jitter: late events, repeats (the drop rule), a jump over several ADUs, large
    inter-event gaps (bit-shifted and full-width residuals), a few wild values."""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, A.EVENT_DTYPE)
    ev["x"] = rng.integers(0, w, n)
    ev["y"] = rng.integers(0, h, n)
    ev["c"] = 0xFF if channels == 1 else rng.integers(0, channels, n)
    ev["d"] = rng.choice(np.array(d_values, np.uint8), n)
    t = np.cumsum(rng.integers(0, 40, n)) + rng.integers(-300, 300, n)
    t[n // 2:] += 40_000
    ev["t"] = np.clip(t, 0, None)
    wild = max(1, n // 80)
    ev["t"][rng.integers(0, n, wild)] = rng.integers(0, 2 ** 31, wild)
    return ev


def _virat():
    """The whole raw sample (one channel, 9-byte big-endian records behind a 25 + 4 * version byte header)."""
    data = open(os.path.join(HERE, "golden", "virat_small_gray.adder"), "rb").read()
    hs = 25 + 4 * min(data[5], 3)
    w, h = struct.unpack(">HH", data[7:11])
    tps, ref, dtm = struct.unpack(">III", data[11:23])
    assert data[23] == 9 and data[24] == 1
    body = np.frombuffer(data[hs: hs + (len(data) - hs) // 9 * 9], np.uint8).reshape(-1, 9).astype(np.uint32)
    x, y = body[:, 0] << 8 | body[:, 1], body[:, 2] << 8 | body[:, 3]
    keep = ~((x == 0xFFFF) & (y == 0xFFFF))  # the EOF event
    ev = np.zeros(int(keep.sum()), A.EVENT_DTYPE)
    ev["x"], ev["y"], ev["c"], ev["d"] = x[keep], y[keep], 0xFF, body[keep, 4]
    ev["t"] = (body[:, 5] << 24 | body[:, 6] << 16 | body[:, 7] << 8 | body[:, 8])[keep]
    return dict(w=int(w), h=int(h), tps=tps, ref=ref, dtm=dtm), ev


def virat_case():
    meta, ev = _virat()
    return dict(name="virat_whole", w=meta["w"], h=meta["h"], c=1, tps=meta["tps"], ref=meta["ref"], dtm=meta["dtm"],
                adu=meta["dtm"] // meta["ref"], cmax=7, header=True, events=lambda: ev)


# ---------------------------------------------------------------- built by hand
def _arms():
    """48x32 (six cubes), ref 100, adu 2 (span 200).  One stream that walks through the arms the seeds may miss."""
    rows = [
        # ADU 0 (start_t 0): cube 0 and cube 2 hit, cube 1 skipped between them
        (3, 3, 0xFF, 7, 150),      # the cube's first: against (d, start_t), |r| >= 127: full
        (4, 3, 0xFF, 5, 10),       # against the previous pixel's first event: negative r, full
        (5, 3, 0xFF, 5, 20),       # short
        (40, 3, 0xFF, 200, 30),    # cube 2; d >= 129
        (3, 3, 0xFF, 7, 150),      # second event not later than the first: kept; delta_t == 0
        (3, 3, 0xFF, 7, 150),      # third, not later: dropped
        (3, 3, 0xFF, 30, 199),     # d_residual beyond 14
        (4, 3, 0xFF, 255, 5),      # second, earlier than the first: kept, clamped to the first's t
        (4, 3, 0xFF, 128, 190),    # previous d == 255: the prediction arm; d == 128
        (4, 3, 0xFF, 3, 200),
        (40, 3, 0xFF, 200, 31),
        (40, 3, 0xFF, 255, 199),
        (40, 3, 0xFF, 1, 200),
        # ADU 1 (start_t 200): an event earlier than start_t, first of its cube: negative r against start_t
        (20, 20, 0xFF, 7, 401),    # closes ADU 0
        (21, 20, 0xFF, 7, 20),     # negative against the previous first event
        (40, 20, 0xFF, 9, 50),     # the first of its cube, earlier than start_t: negative against (d, start_t)
        (3, 3, 0xFF, 7, 402),
    ]
    # a long list in one pixel with growing gaps: every bit shift value
    t = 403
    for k in range(1, 60):
        t += 90 + 37 * k * k
        rows.append((10, 10, 0xFF, 7 + (k % 3), t))
    return events_of(rows)


def _arms_first_negative():
    """The first event of a later ADU's cube is earlier than the ADU's start_t."""
    return events_of([(1, 1, 0xFF, 7, 10), (1, 1, 0xFF, 7, 1000), (2, 2, 0xFF, 7, 5), (1, 1, 0xFF, 7, 1001)])


def _empty_leading():
    """The first event already is past the first ADU's span: that ADU has every cube skipped."""
    return events_of([(1, 1, 0xFF, 7, 2000), (2, 1, 0xFF, 7, 2001), (17, 3, 0xFF, 9, 2100)])


def dense_cut_stream(w, h, channels, n_jump, span, seed=5):
    """Some events, then a jump far ahead: every following event closes an ADU until start_t has caught up."""
    rng = np.random.default_rng(seed)
    n = 40 + n_jump + 60
    ev = np.zeros(n, A.EVENT_DTYPE)
    ev["x"], ev["y"] = rng.integers(0, w, n), rng.integers(0, h, n)
    ev["c"] = 0xFF if channels == 1 else rng.integers(0, channels, n)
    ev["d"] = rng.choice(np.array([3, 7, 8], np.uint8), n)
    t = np.cumsum(rng.integers(0, 5, n))
    t[40:] += (n_jump + 1) * span
    ev["t"] = t
    return ev


def long_list_stream(w, h, n_long, n_mid=65, seed=9):
    """One ADU (the caller's span covers it): one pixel with n_long events, one with n_mid, some others."""
    rng = np.random.default_rng(seed)
    n = n_long + n_mid + 200
    ev = np.zeros(n, A.EVENT_DTYPE)
    ev["x"], ev["y"], ev["c"] = rng.integers(0, w, n), rng.integers(0, h, n), 0xFF
    which = rng.permutation(n)
    ev["x"][which[:n_long]], ev["y"][which[:n_long]] = 5, 6
    ev["x"][which[n_long:n_long + n_mid]], ev["y"][which[n_long:n_long + n_mid]] = w - 1, h - 1
    ev["d"] = rng.choice(np.array([5, 6, 7, 8, 128, 255], np.uint8), n, p=[0.2, 0.2, 0.3, 0.2, 0.05, 0.05])
    ev["t"] = np.cumsum(rng.integers(0, 3, n))  # strictly inside one ADU of 255 * 40 ticks for n < 5000
    return ev


def _case(name, w, h, c, events, *, tps=7650, ref=255, dtm=7650, adu=30, cmax=7, header=True):
    return dict(name=name, w=w, h=h, c=c, tps=tps, ref=ref, dtm=dtm, adu=adu, cmax=cmax, header=header, events=events)


def cpu_cases():
    cases = [
        _case("stream_rs_1", 16, 32, 1, _stream_rs_1, dtm=255 * 5, adu=5, header=False),
        _case("stream_rs_2", 32, 16, 1, _stream_rs_2, dtm=255 * 5, adu=5, header=False),
        _case("stream_rs_3", 30, 30, 1, _stream_rs_3, dtm=2550, adu=10, header=False),
    ]
    for channels, cmax in ((1, 7), (3, 7), (1, 0), (3, 25)):
        seed = channels * 100 + cmax
        cases.append(_case(f"random_c{channels}_m{cmax}", 70, 45, channels,
                           lambda ch=channels, s=seed: random_stream(70, 45, ch, 4000, s), cmax=cmax))
        cases.append(_case(f"random_c{channels}_m{cmax}_adu1", 70, 45, channels,
                           lambda ch=channels, s=seed: random_stream(70, 45, ch, 4000, s)[:1333],
                           tps=5000, ref=100, dtm=100, adu=1, cmax=cmax))
    cases += [
        _case("arms", 48, 32, 1, _arms, tps=1000, ref=100, dtm=200, adu=2),
        _case("arms_first_negative", 16, 16, 1, _arms_first_negative, tps=1000, ref=100, dtm=200, adu=2),
        _case("empty_leading", 33, 17, 1, _empty_leading, tps=1000, ref=100, dtm=200, adu=2),
        _case("dense_cut", 33, 17, 1, lambda: dense_cut_stream(33, 17, 1, 70, 200), tps=1000, ref=100, dtm=200, adu=2),
        _case("long_list", 17, 33, 1, lambda: long_list_stream(17, 33, 700), dtm=255 * 40, adu=40),
    ]
    if os.path.exists(os.path.join(HERE, "golden", "virat_small_gray.adder")):
        cases.append(virat_case())
    return cases


def gpu_cases():
    """The shapes at which each kernel can still go wrong: one cube; partial cubes on both edges; colour (768-pixel
    cubes); 90 cubes (more than a wave of cubes, more than a block)."""
    return [
        _case("g16_random", 16, 16, 1, lambda: random_stream(16, 16, 1, 1500, 1)),
        _case("g17x33_random_m0", 17, 33, 1, lambda: random_stream(17, 33, 1, 2500, 2), cmax=0),
        _case("g48x32x3_random_m25", 48, 32, 3, lambda: random_stream(48, 32, 3, 4000, 3), cmax=25),
        _case("g160x144_random", 160, 144, 1, lambda: random_stream(160, 144, 1, 9000, 4)),
        _case("g160x144_adu1", 160, 144, 1, lambda: random_stream(160, 144, 1, 3000, 6), tps=5000, ref=100, dtm=100,
              adu=1),
        _case("g_arms", 48, 32, 1, _arms, tps=1000, ref=100, dtm=200, adu=2),
        _case("g_empty_leading", 33, 17, 1, _empty_leading, tps=1000, ref=100, dtm=200, adu=2),
        _case("g_long_lists", 17, 33, 1, lambda: long_list_stream(17, 33, 4900), dtm=255 * 40, adu=40),  # 65 and 4900
        _case("g_dense_300", 48, 32, 3, lambda: dense_cut_stream(48, 32, 3, 300, 200), tps=1000, ref=100, dtm=200,
              adu=2),
    ]


# ---------------------------------------------------------------- the logic header's serial driver
def build_sim(tmpdir, extra=()):
    exe = os.path.join(str(tmpdir), "compressed_model_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", *extra, SIM_SRC, "-o", exe])
    return exe


def run_sim(exe, case, events, tmpdir, cut_lanes=64):
    """-> {"start_t", "symbols": [per ADU uint16 arrays], "events": [per ADU EVENT_DTYPE arrays], "events_in",
    "dropped", "bitshift"} from the logic header run serially."""
    fin, fout = os.path.join(str(tmpdir), "case.bin"), os.path.join(str(tmpdir), "case.out")
    ev = np.ascontiguousarray(events, dtype=A.EVENT_DTYPE)
    with open(fin, "wb") as f:
        f.write(struct.pack("<8IQ", case["w"], case["h"], case["c"], case["ref"], case["adu"], case["cmax"], cut_lanes,
                            0, len(ev)))
        f.write(ev.tobytes())
    subprocess.check_call([exe, "model", fin, fout])
    data = open(fout, "rb").read()
    (n_adus,), pos = struct.unpack_from("<Q", data, 0), 8
    out = {"start_t": [], "symbols": [], "events": []}
    for _ in range(n_adus):
        start_t, _z, ns, ne = struct.unpack_from("<IIQQ", data, pos)
        pos += 24
        out["start_t"].append(start_t)
        out["symbols"].append(np.frombuffer(data, np.uint16, ns, pos).copy())
        pos += 2 * ns
        out["events"].append(np.frombuffer(data, A.EVENT_DTYPE, ne, pos).copy())
        pos += 12 * ne
    tail = struct.unpack_from("<18Q", data, pos)
    out["events_in"], out["dropped"], out["bitshift"] = tail[0], tail[1], list(tail[2:])
    return out


def encoder_for(case, threads=1):
    return A.CompressedEncoder(case["w"], case["h"], case["c"], tps=case["tps"], ref_interval=case["ref"],
                               delta_t_max=case["dtm"], adu_interval=case["adu"], c_thresh_max=case["cmax"],
                               write_header=case["header"], threads=threads)


def host_stream(case, events, threads=1):
    """The existing sink's stream for the events."""
    enc = encoder_for(case, threads)
    enc.ingest(events)
    out = enc.close()
    enc.destroy()
    return out


def symbol_stream(case, per_adu_symbols, threads=1):
    enc = encoder_for(case, threads)
    for s in per_adu_symbols:
        enc.ingest_symbols(s)
    out = enc.close()
    enc.destroy()
    return out


def decode(case, stream):
    dec, _ = A.compressed_decode(stream, has_header=case["header"], width=case["w"], height=case["h"],
                                 channels=case["c"], ref_interval=case["ref"], adu_interval=case["adu"])
    return dec
