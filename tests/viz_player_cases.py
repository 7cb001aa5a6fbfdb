"""Seeded streams for the adder-viz player's tests, the committed C checker driven through the literal `consume` loop,
and the configurations both the CPU and the GPU tests use -- test helper.

The generator: every unit has a clock of its own and a speed; whole rows may lag (a low speed for all their units),
units may arrive in bursts (several events of one unit back to back), some units and rows never fire, and D_EMPTY
records are mixed in.  AbsoluteT streams add events from a unit's past (t <= the unit's clock), some of them right
after the unit ran far ahead.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
from viz_player_oracle import EVENT_DTYPE, DELTA_T, ABSOLUTE_T, D_EMPTY

FRAMED_U8, DVS = 0, 6


def gen_stream(seed, width, height, channels, n_events, *, time_mode=DELTA_T, ref_interval=255, max_step=3,
               lag_rows=0.4, burst=0.25, silent_units=0.0, silent_rows=(), past=0.0, d_empty=0.05):
    rng = np.random.default_rng(seed)
    n_units = width * height * channels
    speed = rng.uniform(0.5, 1.0, n_units)
    row_of = np.arange(n_units) // (width * channels)
    for r in range(height):
        if rng.random() < lag_rows:
            speed[row_of == r] *= rng.uniform(0.05, 0.3)
    alive = rng.random(n_units) >= silent_units
    for r in silent_rows:
        alive[row_of == r] = False
    if not alive.any():
        alive[0] = True
    prob = np.where(alive, speed, 0.0)
    prob /= prob.sum()
    clock = np.zeros(n_units, np.int64)
    ev = np.zeros(n_events, EVENT_DTYPE)
    i = 0
    while i < n_events:
        u = int(rng.choice(n_units, p=prob))
        reps = int(rng.integers(2, 7)) if rng.random() < burst else 1
        for _ in range(reps):
            if i >= n_events:
                break
            y, rem = divmod(u, width * channels)
            x, c = divmod(rem, channels)
            d = D_EMPTY if rng.random() < d_empty else int(rng.integers(0, 9))
            if time_mode == ABSOLUTE_T and clock[u] > 0 and rng.random() < past:
                t = int(rng.integers(1, clock[u] + 1))  # from the unit's past: changes nothing
            else:
                step = int(rng.integers(1, max_step * ref_interval + 1))
                if rng.random() < 0.5:
                    step = int(rng.integers(1, max_step + 1)) * ref_interval
                if time_mode == ABSOLUTE_T:
                    clock[u] += step
                    t = int(clock[u])
                else:
                    clock[u] += step  # (the framer's own clock also rounds up; this one only shapes the stream)
                    t = step
            ev[i] = (x, y, c if channels > 1 else 0xFF, d, 0, t)
            i += 1
    return ev


def c_checker_frames(events, cfg, finish=True):
    """The committed C checker (oracle/adder_framer_oracle.c) through the literal consume loop and the flush loop:
    -> [(P, popped-form bytes as uint8 array)]"""
    w, h, c = cfg["width"], cfg["height"], cfg["channels"]
    fr = O.Framer(w, h, c, chunk_rows=1, tps=cfg["tps"], ref_interval=cfg["ref_interval"],
                  delta_t_max=cfg["delta_t_max"], output_fps=cfg["output_fps"], codec_version=cfg["codec_version"],
                  time_mode=cfg["time_mode"], source_camera=cfg["source_camera"])
    if cfg.get("view_mode", 0) or cfg.get("source_type", 0):
        fr.set_view(cfg.get("view_mode", 0), cfg.get("source_type", 0), cfg.get("practical_d_max", 0.0))
    L = fr.L
    limit = cfg["buffer_limit"]
    L.oracle_framer_buffer_limit(fr.h, 0 if limit is None else 1, limit or 0)
    out = []
    n_done = 0

    def show():
        while L.oracle_framer_is_frame_0_filled(fr.h):
            out.append((n_done - 1, np.frombuffer(fr.write_frame_bytes(), np.uint8)))

    evs = np.ascontiguousarray(events, dtype=EVENT_DTYPE).copy()
    p = evs.ctypes.data
    for i in range(len(evs)):
        filled = L.oracle_framer_ingest_event(fr.h, p + 12 * i)
        n_done += 1
        if filled:
            show()
    if finish:
        while fr.flush_frame_buffer():
            show()
    return out


def base_cfg(width, height, channels, *, time_mode=DELTA_T, source_camera=FRAMED_U8, buffer_limit=2, tps=255 * 30,
             ref_interval=255, delta_t_max=255 * 40, output_fps=30.0, codec_version=2, view_mode=0, source_type=0,
             practical_d_max=0.0):
    return dict(width=width, height=height, channels=channels, time_mode=time_mode, source_camera=source_camera,
                buffer_limit=buffer_limit, tps=tps, ref_interval=ref_interval, delta_t_max=delta_t_max,
                output_fps=output_fps, codec_version=codec_version, view_mode=view_mode, source_type=source_type,
                practical_d_max=practical_d_max)


def seeded_set():
    """(name, cfg, events) of the seeded streams the CPU tests run: DeltaT and AbsoluteT (codec_version 2), framed and
    DVS cameras (round-up on and off), a tpf that does not divide ref_interval, D_EMPTY records, limits 1, 2, 3, 60 and
    None."""
    out = []
    seed = 1000
    planes = [(1, 1, 1), (3, 2, 1), (5, 3, 1), (2, 4, 3), (4, 3, 1)]
    for limit in (1, 2, 3, 60, None):
        for time_mode in (DELTA_T, ABSOLUTE_T):
            for cam in (FRAMED_U8, DVS):
                for fps in (30.0, 47.0):  # tpf 255 = ref_interval; tpf 162 does not divide it
                    w, h, c = planes[seed % len(planes)]
                    cfg = base_cfg(w, h, c, time_mode=time_mode, source_camera=cam, buffer_limit=limit, output_fps=fps)
                    ev = gen_stream(seed, w, h, c, 60 + 25 * w * h * c, time_mode=time_mode,
                                    past=0.15 if time_mode == ABSOLUTE_T else 0.0,
                                    silent_units=0.1 if seed % 3 == 0 else 0.0)
                    out.append((f"s{seed}-lim{limit}-tm{time_mode}-cam{cam}-fps{fps:g}-{w}x{h}x{c}", cfg, ev))
                    seed += 1
    # the other view arms, once each
    for view, pdm in ((1, 6.5), (2, 0.0), (3, 0.0)):
        cfg = base_cfg(3, 2, 1, time_mode=ABSOLUTE_T, buffer_limit=2, view_mode=view, practical_d_max=pdm)
        out.append((f"s{seed}-view{view}", cfg, gen_stream(seed, 3, 2, 1, 200, time_mode=ABSOLUTE_T, past=0.1)))
        seed += 1
    return out


def player_kwargs(cfg):
    """cfg -> keyword arguments of HipVizPlayer / VizRestatement"""
    return dict(cfg)


def random_splits(rng, n, pieces):
    """cut points of [0, n) with empty and one-record pieces among them"""
    cuts = sorted(int(x) for x in rng.integers(0, n + 1, pieces))
    cuts = [0] + cuts + [n]
    if n > 3:
        cuts += [cuts[2], min(cuts[2] + 1, n)]  # an empty and a one-record call
    return sorted(cuts)


def gen_sweep(seed, width, height, channels, n_events, *, time_mode=DELTA_T, ref_interval=255, slow_rows=0.3,
              slow_units=0.05, silent_units=0.0, silent_rows=(), past=0.0, jitter=0.3, d_empty=0.05):
    """A camera-like stream: source frame after source frame, every unit fires in a frame with a probability of its
    own (most are 1 or near it: they keep up and frames complete naturally; slow rows and slow units fall behind until a buffer
    limit forces frames out, and their next event arrives late for them), in a fresh random order per frame."""
    rng = np.random.default_rng(seed)
    n_units = width * height * channels
    row_of = np.arange(n_units) // (width * channels)
    fire = np.where(rng.random(n_units) < 0.8, 1.0, rng.uniform(0.85, 1.0, n_units))
    keep_up = fire.copy()  # the first third of the stream: nobody is slow yet, frames complete naturally
    k_slow = max(n_events // (3 * n_units), 2)
    for r in range(height):
        if rng.random() < slow_rows:
            fire[row_of == r] *= rng.uniform(0.05, 0.4)
    fire[rng.random(n_units) < slow_units] *= 0.1
    silent = rng.random(n_units) < silent_units
    for f in (fire, keep_up):
        f[silent] = 0.0
        for r in silent_rows:
            f[row_of == r] = 0.0
    last = np.zeros(n_units, np.int64)  # the unit's clock, in ticks
    ev = np.zeros(n_events, EVENT_DTYPE)
    i, k = 0, 0
    while i < n_events:
        k += 1
        for u in rng.permutation(n_units):
            if i >= n_events:
                break
            if rng.random() >= (keep_up[u] if k < k_slow else fire[u]):
                continue
            now = k * ref_interval - (int(rng.integers(0, ref_interval)) if rng.random() < jitter else 0)
            if now <= last[u]:
                continue
            y, rem = divmod(int(u), width * channels)
            x, c = divmod(rem, channels)
            d = D_EMPTY if rng.random() < d_empty else int(rng.integers(0, 9))
            if time_mode == ABSOLUTE_T and last[u] > 0 and rng.random() < past:
                t = int(rng.integers(1, last[u] + 1))  # from the unit's past
            else:
                t = now if time_mode == ABSOLUTE_T else now - int(last[u])
                last[u] = now
            ev[i] = (x, y, c if channels > 1 else 0xFF, d, 0, t)
            i += 1
    return ev
