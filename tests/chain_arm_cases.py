"""Constructed inputs that take every arm of the Prophesee and DVS chain kernels (the arms: tests/chain_arms.py).
Seeded and deterministic; tests/test_chain_arms_cpu.py holds them to the census condition on the CPU,
tests/test_gpu_chain_arms.py runs them on the device.

Prophesee (prophesee_case): a 16 x 12 plane, about 3700 records over seven view intervals.  Ten pixels carry the
constructed runs, four stay untouched, every other pixel has plain random filler (2 % of it late), so the constructed
pixels' runs start and end inside the sorted order:
  * runs of 48 positive / 66 negative records at successive t, one across each of four group boundaries (the record
    at limit + 1 closes the group and belongs to it, so the next limit is known): step_no_gap, and the clamp of the
    second step three times a run (15 x 0.02 above ln 2 - ln_mid, 21 x 0.02 below -ln_mid);
  * bursts of 18 positive / 24 negative records at one t (same_t: ln leaves the range unclamped), then a record 2..5
    ticks later (the clamp of the gap step) and a late record (skip); one burst of each sign starts a group;
  * the same bursts followed one tick later: no gap step, the second step clamps after theta has been applied.
The time cases shift the whole shape: A starts at t = 2; B so that step times and f32 running times pass 2^24;
C past 2^31; D (ref_time 20) so that each pixel's first gap * ref_time and the end span wrap u32.

DVS (dvs_case): a 6 x 5 plane, about 3700 events.  Six units carry cycles of (set-up event, window event) pairs, the
other units random filler.  The set-up event fires and leaves ln where one window arm needs it; the window event
has an intensity of ln_1p(128 / 255) = 0.40678.  ref 128 reaches it with a zero delta (d = 0), which the same-time
arms need; ref 255 only with a moved time (d = 7, t' = 255), so its cases reach win_hi and win_lo alone.
"""
import numpy as np

import adder_stream_np as S
import prophesee_oracle as PR
from adder_amd import prophesee as P

V = PR.VIEW_INTERVAL

# ---- Prophesee ----------------------------------------------------------------------------------------------------
PPH_W, PPH_H = 16, 12
PPH_T0 = {("A", 1): 2, ("A", 20): 2, ("B", 1): 20_000_000, ("B", 20): 1_000_000, ("C", 1): (1 << 31) + 1000,
          ("C", 20): (1 << 31) // 20 + 1000, ("D", 20): (1 << 32) // 20 + 1000}
PPH_CASES = [(k, r, c) for (k, r) in PPH_T0 for c in (None, 3)]
# (not pixel 0 -- the last record's -- and not the last one: filler pixels sort before and after them)
PPH_PIXELS = dict(H1=37, L1=58, G1=77, K1=101, H2=122, L2=140, G2=163, K2=185, M1=90, M2=45)
PPH_UNTOUCHED = (3, 95, 150, 190)  # no record at all: their end span is the whole recording


def pph_boundary(k):
    """Relative time of the k-th group limit: the record at limit + 1 closes the group, the next starts there."""
    return V + k * (V + 1)


def pph_arms(kind, ref_time):
    """The arms a case is meant to reach."""
    arms = ["skip", "same_t", "step_no_gap", "gap", "gap_clamp_hi", "gap_clamp_lo", "step_clamp_hi", "step_clamp_lo"]
    if kind in "BC":
        arms.append("t_over_2p24")
    if kind == "C":
        arms.append("t_over_2p31")
    if kind == "D":  # (the wrapped products are small again: D has no long step)
        arms += ["gap_time_wrap", "end_span_wrap"]
    return arms


def prophesee_case(kind, ref_time, seed=0):
    """-> dict(recs, W, H, t0, cuts: name -> record index, runs: name -> (first, last) record index,
    bad_at: an index in the middle of a clamp run)."""
    W, H = PPH_W, PPH_H
    t0 = PPH_T0[(kind, ref_time)]
    rng = np.random.default_rng(1000 + seed)
    items = []  # (sort time, priority, sequence, relative t, pixel, polarity, tag)

    def add(pos, r, px, p, tag, prio=0):
        items.append((pos, prio, len(items), r, px, p, tag))

    def run(name, start, n, p):
        for i in range(n):
            add(start + i, start + i, PPH_PIXELS[name], p, (name, "run", start, i))

    def burst(name, r, n, p, follow):
        px = PPH_PIXELS[name]
        for i in range(n):
            add(r, r, px, p, (name, "burst", r, i))
        add(r + follow, r + follow, px, p, (name, "follow", r, 0))
        add(r + follow, r - 1, px, 1 - p, (name, "late", r, 0))  # t below the pixel's last t: skipped

    B = pph_boundary
    run("H1", B(0) - 20, 48, 1)
    run("L1", B(1) - 30, 66, 0)
    run("H2", B(4) - 40, 48, 1)
    run("L2", B(5) - 7, 66, 0)
    for name, n, p, at in (("G1", 18, 1, (B(2) + 1, B(2) + 2001, B(2) + 4001)), ("K1", 24, 0, (B(3) + 1, B(3) + 3001, B(3) + 5001)),
                           ("G2", 18, 1, (7000, 9000, 40000)), ("K2", 24, 0, (11000, 13000, 60000))):
        for j, r in enumerate(at):
            burst(name, r, n, p, (5, 2, 3)[j])
    for j, r in enumerate((20000, 24000, 52000, 56000)):  # no gap after the burst: the second step clamps
        burst("M1", r, 18, 1, 1)
        burst("M2", r + 500, 24, 0, 1)
    end = B(6) + 300
    # filler on every other pixel; the first record at relative time 0 (it closes the first group of a shifted case)
    free = np.array([u for u in range(W * H) if u not in PPH_PIXELS.values() and u not in PPH_UNTOUCHED])
    n_fill = 3000
    fr = np.sort(rng.integers(0, end, n_fill))
    fr[0] = 0
    fpx = free[rng.integers(0, len(free), n_fill)]
    fp = rng.integers(0, 2, n_fill)
    late = rng.random(n_fill) < 0.02
    late[0] = False
    ft = np.where(late, np.maximum(fr - rng.integers(1, 5000, n_fill), 0), fr)
    for pos, r, px, p in zip(fr.tolist(), ft.tolist(), fpx.tolist(), fp.tolist()):
        add(pos, r, px, p, None, prio=1)
    items.sort(key=lambda it: it[:3])
    r = np.array([it[3] for it in items], np.int64)
    px = np.array([it[4] for it in items], np.int64)
    p = np.array([it[5] for it in items], np.int64)
    t = t0 + r
    # the last record one tick after the largest t, so that no pixel's last t equals running_t at the end
    t, px, p = np.append(t, t.max() + 1), np.append(px, 0), np.append(p, 1)
    assert int(t.max()) < (1 << 32)
    runs, where = {}, {}
    for i, it in enumerate(items):
        tag = it[6]
        if tag is None:
            continue
        where[tag] = i
        if tag[1] in ("run", "burst"):
            key = (tag[0], tag[2])
            a, b = runs.get(key, (i, i))
            runs[key] = (min(a, i), max(b, i))
    cuts = dict(
        after_same_t_burst=where[("G2", "burst", 7000, 17)] + 1,  # the burst's follow-up record starts the next push
        inside_clamp_run=where[("H1", "run", B(0) - 20, 10)],
        inside_burst=where[("K2", "burst", 11000, 12)],
        inside_negative_run=where[("L1", "run", B(1) - 30, 20)] + 1,
        after_group_opening_burst=where[("K1", "burst", B(3) + 1, 23)] + 1,
    )
    return dict(recs=P.records(t, px % W, px // W, p), W=W, H=H, t0=t0, cuts=cuts, runs=runs,
                bad_at=where[("H2", "run", B(4) - 40, 12)])


# ---- DVS ----------------------------------------------------------------------------------------------------------
DVS_W, DVS_H = 6, 5
DVS_CAM = 6  # SourceCamera::Dvs: not framed
DVS_CASES = [(tm, ch, cam, ref) for tm in (0, 1) for ch in (1, 3) for cam in (0, DVS_CAM) for ref in (255, 128)]
DVS_THETAS = (0.01, 0.3)
DVS_UNITS = ((2, 1), (4, 1), (1, 2), (3, 2), (5, 3), (2, 3))  # (x, y); channel 1 of three
# set-up events (d, t') per ref, by the arm the window event after them takes at theta 0.01
DVS_SETUP = {
    128: dict(win_hi=(8, 128), win_same_hi=(4, 9), win_lo=(128, 5), win_same_lo=(0, 2)),
    255: dict(win_hi=(8, 255), win_lo=(128, 5)),
}
DVS_WINDOW_MOVED = {128: (7, 128), 255: (7, 255)}  # the window intensity after a moved time
DVS_WINDOW_SAME = (0, 0)  # ref 128 only: the window intensity with a zero delta
# a unit's first event, ref 128: ln in (0.6, win_hi] or [win_lo, 0.3), at a time that is / is not a multiple of ref
DVS_FIRST_128 = ((11, 1152), (4, 9), (7, 256), (0, 2))


def dvs_arms(time_mode, cam, ref, theta):
    """The arms a case is meant to reach at this theta."""
    arms = ["first", "empty", "d128", "t0", "up", "down", "none", "win_hi", "win_lo"]
    if cam != DVS_CAM:
        arms.append("rounded")
    if time_mode == 1:
        arms.append("abs_saturate")
    if ref == 128 and theta == 0.01:  # at theta 0.3 the ranges (0.6, win_hi] and [win_lo, 0.3) are empty
        arms += ["win_same_hi", "win_same_lo"]
    return arms


def dvs_case(time_mode, ch, cam, ref, seed=0):
    """-> dict(meta, ev, pairs: [(set-up index, window index, kind)], first_pairs: the pairs whose set-up event is
    the unit's first event, bad_at: the window index of one pair)."""
    w, h = DVS_W, DVS_H
    rng = np.random.default_rng(2000 + seed + 8 * time_mode + 4 * (ch == 3) + 2 * (cam == DVS_CAM) + (ref == 128))
    framed = cam != DVS_CAM
    c_con = 0xFF if ch == 1 else 1
    con = []  # (unit index, d, t, role, kind)
    for ui in range(len(DVS_UNITS)):
        T = [0]  # the unit's stored time as the conversion keeps it

        def emit(d, dt, role, kind, first=False):
            if first:
                t, T[0] = dt, dt  # the first event's time is stored as it comes
            else:
                t = dt if time_mode == 0 else T[0] + dt
                T[0] = T[0] + dt
                if framed and T[0] % ref:
                    T[0] = (T[0] // ref + 1) * ref
            assert t < (1 << 32)
            con.append((ui, d, t, role, kind))

        kinds = list(DVS_SETUP[ref])
        if ref == 128 and ui < 4:
            # the first event is the set-up event of a same-time pair (dvs_ln_kernel's prev_first branch)
            emit(*DVS_FIRST_128[ui], "setup", "first_same", first=True)
            emit(*DVS_WINDOW_SAME, "window", "first_same")
        else:
            emit(7, 300 + 7 * ui, "other", None, first=True)
        for cyc in range(3):
            for kind in kinds[ui % len(kinds):] + kinds[:ui % len(kinds)]:
                emit(*DVS_SETUP[ref][kind], "setup", kind)
                if cyc == 1 and kind.startswith("win_same"):
                    emit(255, 0 if ui % 2 else 3, "other", None)  # D_EMPTY between the two: the time moves alone
                same = kind.startswith("win_same") or (ref == 128 and (cyc + ui) % 2 == 0)
                emit(*(DVS_WINDOW_SAME if same else DVS_WINDOW_MOVED[ref]), "window", kind)
            if ref == 128:  # a same-time set-up followed by a moved time: the same-time arms must not be taken
                for kind in ("win_same_hi", "win_same_lo"):
                    emit(*DVS_SETUP[ref][kind], "setup", "moved_" + kind)
                    emit(*DVS_WINDOW_MOVED[ref], "window", "moved_" + kind)
    # filler on the other units, in the style of the fuzz streams
    n_fill = 3500
    taken = {(x, y, c_con) for x, y in DVS_UNITS}
    fill = np.zeros(n_fill, S.EVENT_DTYPE)
    k = 0
    seen = set()
    while k < n_fill:
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        c = int(rng.integers(0, ch)) if ch > 1 else 0xFF
        if (x, y, c) in taken:
            continue
        d = int(rng.choice(np.array([0, 1, 2, 3, 5, 7, 8, 9, 12, 20, 40, 127, 128, 255])))
        if (x, y, c) not in seen:  # a unit's first event has d <= 128
            seen.add((x, y, c))
            d = 6 if d == 255 else d
        t = 0 if rng.integers(0, 4) == 0 else int(rng.integers(1, 3000))
        fill[k] = (x, y, c, d, 0, t)
        k += 1
    # the constructed events keep their order and land at random places among the filler
    n = n_fill + len(con)
    slots = np.sort(rng.choice(np.arange(20, n - 20), len(con), replace=False))
    ev = np.zeros(n, S.EVENT_DTYPE)
    is_con = np.zeros(n, bool)
    is_con[slots] = True
    ev[~is_con] = fill
    pairs, first_pairs, last_setup = [], [], {}
    for slot, (ui, d, t, role, kind) in zip(slots.tolist(), con):
        x, y = DVS_UNITS[ui]
        ev[slot] = (x, y, c_con, d, 0, t)
        if role == "setup":
            last_setup[ui] = slot
        elif role == "window":
            pairs.append((last_setup[ui], slot, kind))
            if kind == "first_same":
                first_pairs.append(pairs[-1])
    meta = dict(width=w, height=h, channels=ch, time_mode=time_mode, ref_interval=ref, source_camera=cam)
    bad_at = next(wi for _, wi, kind in pairs if kind == "win_lo")
    return dict(meta=meta, ev=ev, pairs=pairs, first_pairs=first_pairs, bad_at=bad_at)
