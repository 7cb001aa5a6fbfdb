"""Streams, rings and call plans that make the adder-viz player's pending ring wrap -- test helper, CPU only.

The player keeps frame f in slot f % ring and refuses a call in which some fill reaches frame w0 + ring or beyond (w0 =
frames_written when the call starts).  `ahead` measures, with the literal restatement alone, how far any event runs
ahead of frames_written; `plan` cuts a stream into the longest calls a ring of R frames must accept; `census` counts
what such a plan reaches (wraps, two-piece clears, fills on the last slot), so that no test of the wrap passes
vacuously.  Nothing here looks at the product.
"""
import functools

import numpy as np

import viz_player_cases as K
from viz_player_oracle import VizRestatement, unit_chain, DELTA_T, ABSOLUTE_T

# name -> (width, height, channels, events, time mode, limit, camera, output fps, generator options)
_KEEP_UP = dict(slow_rows=0.0, slow_units=0.0)  # every unit keeps up: frames complete naturally, the ring can be tiny
STREAMS = {
    "7x5-abs-lim2": (7, 5, 1, 3000, ABSOLUTE_T, 2, K.FRAMED_U8, 30.0, {}),
    "7x5-abs-lim1": (7, 5, 1, 3000, ABSOLUTE_T, 1, K.FRAMED_U8, 30.0, {}),
    "7x5-abs-dvs-lim3": (7, 5, 1, 3000, ABSOLUTE_T, 3, K.DVS, 30.0, {}),
    "4x3rgb-abs-lim2": (4, 3, 3, 3000, ABSOLUTE_T, 2, K.FRAMED_U8, 30.0, {}),
    "7x5-dt-lim2": (7, 5, 1, 3000, DELTA_T, 2, K.FRAMED_U8, 30.0, {}),
    "7x5-dt-47fps-lim2": (7, 5, 1, 3000, DELTA_T, 2, K.FRAMED_U8, 47.0, {}),
    "3x70-abs-lim2": (3, 70, 1, 8000, ABSOLUTE_T, 2, K.FRAMED_U8, 30.0, dict(slow_rows=0.03)),  # rows past a wave
    # a row past a block; 16 000 events: at ring 5, 12 000 give only one call that clears across the wrap
    "257x3-abs-lim2": (257, 3, 1, 16000, ABSOLUTE_T, 2, K.FRAMED_U8, 30.0, {}),
    "5x4-abs-nolimit": (5, 4, 1, 2000, ABSOLUTE_T, None, K.FRAMED_U8, 30.0, dict(_KEEP_UP, past=0.0)),
    "5x4-dt-nolimit": (5, 4, 1, 2000, DELTA_T, None, K.FRAMED_U8, 30.0, dict(_KEEP_UP)),
}


@functools.lru_cache(maxsize=None)
def stream(name):
    """-> (cfg, events)"""
    w, h, c, n, time_mode, limit, cam, fps, opts = STREAMS[name]
    cfg = K.base_cfg(w, h, c, time_mode=time_mode, buffer_limit=limit, source_camera=cam, output_fps=fps)
    o = dict(slow_rows=0.3, past=0.1 if time_mode == ABSOLUTE_T else 0.0)
    o.update(opts)
    return cfg, K.gen_sweep(1, w, h, c, n, time_mode=time_mode, **o)


def chain(cfg, ev):
    """unit_chain with the configuration's constants: -> row, from, to, L, unit"""
    r = VizRestatement(**cfg)
    return unit_chain(ev, cfg["width"], cfg["channels"], tpf=r.tpf, ref_interval=cfg["ref_interval"], abs_t=r.abs_t,
                      round_up=r.round_up)


_AHEAD = {}


def ahead(cfg, ev, change=None):
    """The restatement fed one event at a time: -> (W, to); W[i] = frames_written before event i (and before the loop
    in front of the read loop, when `change` = (index, limit) lowers the limit right before that event), W[len] = after
    the last; to = unit_chain's.  A ring of R frames can hold the stream only if max(to - W[:-1]) < R."""
    key = (repr(sorted(cfg.items())), ev.tobytes(), change)
    if key not in _AHEAD:
        r = VizRestatement(**cfg)
        W = np.zeros(len(ev) + 1, np.int64)
        for i in range(len(ev)):
            W[i] = r.frames_written
            if change is not None and change[0] == i:
                r.set_buffer_limit(change[1])
            r.feed(ev[i:i + 1])
        W[len(ev)] = r.frames_written
        _AHEAD[key] = (W, chain(cfg, ev)[2].astype(np.int64))
    return _AHEAD[key]


def min_ring(cfg, ev, change=None):
    W, to = ahead(cfg, ev, change)
    return int((to - W[:-1]).max()) + 1


def plan(cfg, ev, R, change=None):
    """Greedy maximal cuts: a call [a, b) is extended while to[b] < W[a] + R, so the player must accept every one of
    them; a lowered limit (`change`) starts a call of its own.  -> cut points, from 0 to len(ev)"""
    W, to = ahead(cfg, ev, change)
    assert int((to - W[:-1]).max()) < R, "no ring of this size holds the stream"
    cuts, a = [0], 0
    for b in range(len(ev)):
        if to[b] >= W[a] + R or (change is not None and b == change[0] and b > a):
            cuts.append(b)
            a = b
    cuts.append(len(ev))
    return cuts


def replay(cfg, ev, cuts, change=None):
    """The restatement fed call by call: -> (restatement after finish, [(a, b, w0, n_pops)] per call, frames before the
    drain)"""
    r = VizRestatement(**cfg)
    calls = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        w0 = r.frames_written
        if change is not None and change[0] == a:
            r.set_buffer_limit(change[1])
        r.feed(ev[a:b])
        calls.append((a, b, w0, r.frames_written - w0))
    before = len(r.popped)
    r.finish()
    return r, calls, before


def census(cfg, ev, R, cuts, change=None):
    """What the plan reaches with a ring of R frames"""
    r, calls, before = replay(cfg, ev, cuts, change)
    _, frm, to, _, _ = chain(cfg, ev)
    across = last_slot = 0
    for a, b, w0, n_pops in calls:
        fills = to[a:b][to[a:b] > frm[a:b]]
        assert not len(fills) or int(fills.max()) < w0 + R
        across += int(w0 % R != 0 and w0 % R + n_pops > R)
        last_slot += int((fills == w0 + R - 1).any())
    return dict(calls=len(calls), before_drain=before, wraps=before // R, across=across, last_slot=last_slot,
                max_pops=max(c[3] for c in calls), with_none=sum(1 for p in r.popped[:before] if not p[2].all()))


# the smallest ring that holds each stream: min_ring(*stream(name)), recorded (test_viz_ring_cpu.py compares)
MIN_RING = {"7x5-abs-lim2": 6, "7x5-abs-lim1": 5, "7x5-abs-dvs-lim3": 7, "4x3rgb-abs-lim2": 4, "7x5-dt-lim2": 26,
            "7x5-dt-47fps-lim2": 37, "3x70-abs-lim2": 10, "257x3-abs-lim2": 4, "5x4-abs-nolimit": 2, "5x4-dt-nolimit": 17}


def cases():
    """every (stream, ring) the wrap tests run: each stream at its smallest ring and at one more"""
    return [(name, MIN_RING[name] + extra) for name in STREAMS for extra in (0, 1)]


def limit_change(cfg, ev, R, cuts, limit=1):
    """-> (index, limit): the limit is lowered in front of the first planned call after the middle of the stream that
    starts at a wrapped frames_written (w0 >= R, w0 % R != 0) and whose ring still holds the stream afterwards"""
    _, calls, _ = replay(cfg, ev, cuts)
    for a, _, w0, _ in calls:
        if a >= len(ev) // 2 and w0 >= R and w0 % R != 0:
            change = (a, limit)
            if min_ring(cfg, ev, change) <= R:
                return change
    return None
