"""Seeded inputs that take the stream tools (include/adder_stream.h, csrc/adder_stream.hip) to their edges, and a census
of each: 11-byte records of every tag, sentinel keys at power-of-two unit counts, batches at the 256-thread grid's edges,
bad and EOF records at both ends of a batch and in both orders, sums at 2^32 - 1 and 2^32, and every arm of the
dynamic-range fold far inside a long stream and on both sides of a batch cut.

A case is a dict: name, group, meta (the INPUT stream's), ops, cuts (batch boundaries in records), `body` (the wire
records, always) and `events` (AdderEvents; None where only the wire can say it -- tags 0 / > 1 with a spare byte),
`breaks` (what the builder put where: the case's claim) and `facts` (further claims of its group).  Everything here is
numpy and the restatement (stream_tools_oracle.py); nothing touches the library.

ops: forward (DeltaT -> AbsoluteT), inverse (AbsoluteT -> DeltaT), pass_same (out mode = in mode), pass_mixed, info.
expected() gives, batch by batch, what include/adder_stream.h promises: the oracle runs on the records in front of the
batch's first end record, stops at its first bad event and keeps the state of the events before it, so the next batch
continues "with the bad event left out" (and with it the rest of its batch)."""
import numpy as np

import adder_stream_np as S
import stream_tools_oracle as R

U32 = (1 << 32) - 1
NONE = 0xFF
DVS_CAM = 6
BLOCK = 256  # threads per block of every kernel in adder_stream.hip
SCAN_SPAN = 4096  # a fold arm at a position >= this has several tiles of the device scan on both sides in 6 000 events
D_POOL = np.array([0, 1, 2, 3, 5, 7, 8, 9, 12, 20, 40, 100, 127, 128, 128, 255, 255], np.uint8)


def meta_of(w, h, ch, version=2, time_mode=0, ref=255, cam=0):
    return dict(width=w, height=h, channels=ch, version=version, time_mode=time_mode, ref_interval=ref,
                source_camera=cam, tps=7650, delta_t_max=2550, adu_interval=0)


def n_units(meta):
    return meta["width"] * meta["height"] * meta["channels"]


def from_units(meta, units, d, t, pad=0):
    """events of the units (y * width + x) * channels + c; a one-channel plane's c is None"""
    w, ch = meta["width"], meta["channels"]
    units = np.asarray(units, np.int64)
    ev = np.zeros(len(units), S.EVENT_DTYPE)
    ev["c"] = units % ch if ch > 1 else NONE
    ev["x"], ev["y"] = (units // ch) % w, units // ch // w
    ev["d"], ev["t"], ev["pad"] = d, t, pad
    return ev


def unit_of(meta, ev):
    """unit index per event, -1 outside the plane (c = None counts as channel 0)"""
    c = np.where(ev["c"] == NONE, 0, ev["c"]).astype(np.int64)
    inside = (ev["x"] < meta["width"]) & (ev["y"] < meta["height"]) & (c < meta["channels"])
    u = (ev["y"].astype(np.int64) * meta["width"] + ev["x"]) * meta["channels"] + c
    return np.where(inside, u, -1)


def random_events(rng, meta, n, units=None, hot=0.3, t_hi=3000):
    """DeltaT events: unit 0 owns a share `hot` of them; d from the old fuzz's pool; a fifth of the times are 0"""
    units = rng.integers(0, n_units(meta), n) if units is None else np.asarray(units)
    units = np.where(rng.random(n) < hot, 0, units)
    t = np.where(rng.integers(0, 5, n) == 0, 0, rng.integers(1, t_hi, n))
    return from_units(meta, units, rng.choice(D_POOL, n), t, rng.integers(0, 1 << 16, n))


def with_times(ev, out):
    got = ev[: len(out)].copy()
    if len(out):
        a = np.array(out, dtype=np.int64)
        assert np.array_equal(a[:, 0], got["x"]) and np.array_equal(a[:, 1], got["y"]) and \
            np.array_equal(a[:, 2], got["c"]) and np.array_equal(a[:, 3], got["d"])
        got["t"] = a[:, 4]
    return got


def to_absolute(meta, ev):
    """the AbsoluteT stream migrate_v2 makes of a clean DeltaT stream with this ref and camera"""
    out, bad = R.Migration(dict(meta, time_mode=0), R.ABSOLUTE_T).run(ev)
    assert bad is None
    return with_times(ev, out)


OPS_DT = ("forward", "pass_same", "pass_mixed", "info")
OPS_ABS = ("inverse", "pass_same", "pass_mixed", "info")


def out_mode(meta, op):
    return {"forward": R.ABSOLUTE_T, "inverse": R.DELTA_T, "pass_mixed": R.MIXED,
            "pass_same": R.in_time_mode(meta)}[op]


def make_oracle(meta, op):
    if op == "info":
        return R.Info(meta)
    m = R.Migration(meta, out_mode(meta, op))
    assert m.direction == (op if op in ("forward", "inverse") else "pass"), (op, m.direction)
    return m


def case(name, group, meta, ops, cuts, events=None, body=None, breaks=(), facts=None):
    if body is None:
        body = S.encode_records(events, meta["channels"])
    rb = 9 if meta["channels"] == 1 else 11
    n = len(body) // rb
    assert len(body) == n * rb and (events is None or len(events) == n)
    assert cuts[0] == 0 and cuts[-1] == n and all(a <= b for a, b in zip(cuts[:-1], cuts[1:]))
    return dict(name=name, group=group, meta=meta, ops=tuple(ops), cuts=tuple(int(c) for c in cuts), events=events,
                body=body, breaks=tuple(breaks), facts=facts or {}, n=n, record_bytes=rb)


def apply_breaks(meta, ev, breaks, absolute):
    """-> (events, body) with the breaks put in.  kinds: oop (x = width), eof (x = y = 0xFFFF), tag (byte 4 of the
    wire record; the events cannot say it), c (channel byte), cx (the channel byte in the events, x = width in the wire
    record, which may have no channel byte), time (DeltaT: t = 2^32 - 1 on a unit whose T is >= 1;
    AbsoluteT: t = 0 on a unit whose previous time is >= 1)."""
    ev = ev.copy()
    only_wire = False
    for b in breaks:
        i, kind = b["i"], b["kind"]
        if kind == "oop":
            ev["x"][i] = meta["width"]
        elif kind == "eof":
            ev["x"][i] = ev["y"][i] = 0xFFFF
        elif kind in ("c", "cx"):
            ev["c"][i] = b["arg"]
        elif kind == "time":
            ev["t"][i] = 0 if absolute else U32
        else:
            assert kind == "tag"
            only_wire = True
    rb = 9 if meta["channels"] == 1 else 11
    body = bytearray(S.encode_records(ev, meta["channels"]))
    for b in breaks:
        if b["kind"] == "tag":
            body[11 * b["i"] + 4] = b["arg"]
        if b["kind"] == "cx":
            body[rb * b["i"]:rb * b["i"] + 2] = bytes([meta["width"] >> 8, meta["width"] & 0xFF])
    return (None if only_wire else ev), bytes(body)


def claimed(c, op, source):
    """From the breaks alone: per batch (bad index or None, records consumed) -- both within the batch."""
    meta = c["meta"]
    absolute = R.in_time_mode(meta) == R.ABSOLUTE_T
    info_abs = meta["version"] >= 2 and meta["time_mode"] == R.ABSOLUTE_T
    out = []
    for a, b in zip(c["cuts"][:-1], c["cuts"][1:]):
        end, bad = b - a, None
        for br in sorted(c["breaks"], key=lambda br: br["i"]):
            i, kind = br["i"] - a, br["kind"]
            if not 0 <= i < end:
                continue
            is_end = source == "wire" and (kind == "tag" or kind == "eof")
            if kind in ("oop", "cx") or (kind == "eof" and source == "events"):
                is_bad = True
            elif kind == "c":
                arg = 0 if br["arg"] == NONE else br["arg"]
                is_bad = arg >= meta["channels"] and (source == "events" or meta["channels"] > 1)
            elif kind in ("time", "timebad"):
                ops = br.get("ops") or (("inverse", "info") if absolute else ("forward",))
                is_bad = op in ops and (op != "info" or info_abs)
            else:
                is_bad = False
            if is_end:
                end = i
                break
            if is_bad and bad is None:
                bad = i  # the end record behind it still ends what was consumed
        out.append((bad, end))
    return out


def scanned(c, source):
    """From the records alone, in numpy: per batch (first record outside the plane in front of the end, or None;
    the first end record, or the batch's length)."""
    meta, rb, out = c["meta"], c["record_bytes"], []
    for a, b in zip(c["cuts"][:-1], c["cuts"][1:]):
        if source == "wire":
            ev, _, _, end = S.decode_records(c["body"][rb * a:rb * b], meta["channels"])
        else:
            ev, end = c["events"][a:b], b - a
        oop = np.flatnonzero(unit_of(meta, ev[:end]) < 0)
        out.append((int(oop[0]) if len(oop) else None, end))
    return out


_EXPECTED = {}


def expected(c, op, source):
    """-> per batch dict(n, bad, consumed, done, rc, out (the migrated records before `done`, as bytes), range)."""
    key = (c["name"], op, source)
    if key in _EXPECTED:
        return _EXPECTED[key]
    meta, rb = c["meta"], c["record_bytes"]
    orc, res = make_oracle(meta, op), []
    for a, b in zip(c["cuts"][:-1], c["cuts"][1:]):
        if source == "wire":
            ev, tag, spare, end = S.decode_records(c["body"][rb * a:rb * b], meta["channels"])
        else:
            ev, end = c["events"][a:b], b - a
        r = dict(n=b - a, consumed=end)
        if op == "info":
            bad, out = orc.run(ev[:end]), b""
        else:
            got, bad = orc.run(ev[:end])
            got = with_times(ev, got)
            out = got.tobytes() if source == "events" else \
                S.encode_records(got, meta["channels"], tag[: len(got)], spare[: len(got)])
        r.update(bad=bad, done=end if bad is None else bad, rc=0 if bad is None else -20, out=out)
        if op == "info":
            r["range"] = (orc.min, orc.max, orc.count)
        res.append(r)
    _EXPECTED[key] = res
    return res


def pair(name, group, meta, dt_events, cuts, breaks=(), facts=None, ops_dt=OPS_DT, ops_abs=OPS_ABS, tags=None):
    """the DeltaT case and the AbsoluteT case of one clean DeltaT stream, the same breaks put into both.  tags:
    (tag, spare) arrays for the wire body (RGB; c of a tag-0 record is None)."""
    out = []
    for absolute in (False, True):
        m = dict(meta, time_mode=1 if absolute else 0)
        ev = to_absolute(m, dt_events) if absolute else dt_events
        ev, body = apply_breaks(m, ev, breaks, absolute)
        if tags is not None:
            src, _ = apply_breaks(m, to_absolute(m, dt_events) if absolute else dt_events,
                                  [b for b in breaks if b["kind"] != "tag"], absolute)
            body = bytearray(S.encode_records(src, 3, tags[0], tags[1]))
            for b in breaks:
                if b["kind"] == "tag":
                    body[11 * b["i"] + 4] = b["arg"]
            ev, body = None, bytes(body)
        out.append(case(f"{name}/{'abs' if absolute else 'dt'}", group, m, ops_abs if absolute else ops_dt, cuts,
                        events=ev, body=body, breaks=breaks, facts=facts))
    return out


def br(i, kind, arg=None, ops=None):
    return dict(i=int(i), kind=kind, arg=arg, ops=ops)


# ---- wire11 tags ----------------------------------------------------------------------------------------------------

def tag_cases():
    meta = meta_of(6, 5, 3)
    n, cut = 700, 450
    out = []
    variants = (("mixed", ()), ("end_tag2", (br(400, "tag", 2),)), ("end_tag255", (br(400, "tag", 255),)),
                ("tag9_then_eof", (br(300, "tag", 9), br(500, "eof"))), ("eof_then_tag7", (br(300, "eof"), br(500, "tag", 7))))
    for k, (name, breaks) in enumerate(variants):
        rng = np.random.default_rng([11, k])
        ev = random_events(rng, meta, n)
        tag0 = (ev["c"] == 0) & (rng.random(n) < 0.6)  # None counts as channel 0
        ev["c"][tag0] = NONE
        spare = np.where(tag0, rng.integers(1, 256, n), 0).astype(np.uint8)
        out += pair(f"tags_{name}", "tags", meta, ev, (0, cut, n), breaks, tags=(np.where(tag0, 0, 1), spare),
                    facts=dict(tag0=int(tag0.sum())))
    return out


# ---- unit counts ----------------------------------------------------------------------------------------------------

UNIT_PLANES = ((1, 1, 1), (16, 16, 1), (5, 17, 3), (8, 8, 1), (32, 32, 1))


def unit_cases():
    out = []
    for k, (w, h, ch) in enumerate(UNIT_PLANES):
        meta = meta_of(w, h, ch)
        rng = np.random.default_rng([12, k])
        n, p_oop, cut, p_eof = 600, 200, 300, 450
        units = rng.integers(0, n_units(meta), n)
        units[-1] = n_units(meta) - 1  # the last unit, next to the sentinel keys in sorted order
        ev = random_events(rng, meta, n, units)
        for p in (p_oop - 1, p_oop + 1, p_eof - 1, p_eof + 1):  # unit 0 on both sides of every sentinel
            ev[p] = from_units(meta, [0], 5, 17)[0]
        # 8x8x1: the record outside the plane is a three-channel event (c = 2) in the events, x = width in the wire
        breaks = (br(p_oop, "cx", 2) if (w, h) == (8, 8) else br(p_oop, "oop"), br(p_eof, "eof"))
        out += pair(f"units_{w}x{h}x{ch}", "units", meta, ev, (0, cut, n), breaks,
                    ops_dt=("forward", "info"), ops_abs=("inverse", "info"), facts=dict(p_oop=p_oop, p_eof=p_eof))
    return out


# ---- grid edges -----------------------------------------------------------------------------------------------------

GRID_N = (1, 2, 255, 256, 257, 511, 512, 513, 1025)
FOLLOW = 9  # events of the second batch: the state after the first


def heads_histogram(n, units):
    """sorted position -> unit: runs [0, 255), {255}, [256, 512), [512, n - 1), {n - 1} as far as n goes, so that a
    run's head sits on thread 0 of the second and third block and single-event runs on the last thread of the first
    block and at the very end"""
    pos = np.arange(n)
    u = np.select([pos == n - 1, pos < 255, pos == 255, pos < 512], [units - 1, 0, 1, 2], 3)
    return u


def span_histogram(n, units):
    """[0, 200) unit 0, [200, 801) unit 1 -- over more than two blocks --, then runs of one event"""
    pos = np.arange(n)
    assert n - 801 <= units - 2
    return np.where(pos < 200, 0, np.where(pos <= 800, 1, 2 + pos - 801))


def grid_cases():
    out = []
    for n in GRID_N + ("span",):
        if n == "span":
            meta, n, name = meta_of(16, 5, 3), 1025, "grid_span_1025"
            hist = span_histogram(n, n_units(meta))
        else:
            meta, name = meta_of(4, 4, 1), f"grid_heads_{n}"
            hist = heads_histogram(n, n_units(meta))
        rng = np.random.default_rng([13, n, len(name)])
        units = np.concatenate([rng.permutation(hist), rng.choice(hist, FOLLOW)])
        ev = random_events(rng, meta, n + FOLLOW, units, hot=0.0)
        out += pair(name, "grid", meta, ev, (0, n, n + FOLLOW), ops_dt=("forward", "info"),
                    ops_abs=("inverse", "info"), facts=dict(n=n, histogram=hist))
    return out


def sorted_keys(c, batch=0):
    """the keys of a batch in the order the device's stable sort leaves them (out-of-plane and end records last)"""
    a, b = c["cuts"][batch], c["cuts"][batch + 1]
    ev, _, _, end = S.decode_records(c["body"][c["record_bytes"] * a:c["record_bytes"] * b], c["meta"]["channels"])
    u = unit_of(c["meta"], ev)
    u[end:end + 1] = -1
    u = np.where(u < 0, n_units(c["meta"]), u)
    return np.sort(u, kind="stable")


# ---- error interplay ------------------------------------------------------------------------------------------------

def error_cases():
    """300 records (two blocks) with the breaks, then a clean batch of 100.  Units 0 and 1 of the plane are kept for the
    time breaks: an event with t = 100 first, so that T >= 1 (DeltaT) and the previous time is >= 1 (AbsoluteT)."""
    out = []
    n1, n = 300, 400

    def stream(seed, meta, early=(10, 20)):
        rng = np.random.default_rng([14, seed])
        ev = random_events(rng, meta, n, rng.integers(2, n_units(meta), n), hot=0.0)
        for u, i in enumerate(early):
            ev[i] = from_units(meta, [u], 5, 100)[0]
        for u, i in enumerate((n1 + 10, n1 + 20)):  # the reserved units again in the second batch: their state
            ev[i] = from_units(meta, [u], 5, 50_000)[0]
        return ev

    def place(ev, meta, i, unit):
        ev[i] = from_units(meta, [unit], 5, 60)[0]

    gray, rgb = meta_of(4, 3, 1, ref=5000), meta_of(4, 3, 3, ref=5000)
    plain = (("bad_at_0", (br(0, "oop"),)), ("bad_at_last", (br(n1 - 1, "oop"),)),
             ("eof_at_0", (br(0, "eof"),)), ("eof_at_last", (br(n1 - 1, "eof"),)),
             ("eof_then_bad", (br(100, "eof"), br(200, "oop"))), ("bad_then_eof", (br(100, "oop"), br(200, "eof"))),
             ("bad_and_eof_in_second_batch", (br(n1, "oop"), br(n - 1, "eof"))))
    for k, (name, breaks) in enumerate(plain):
        for meta in (gray, rgb):
            out += pair(f"err_{name}_{meta['channels']}ch", "errors", meta, stream(k, meta), (0, n1, n), breaks,
                        ops_dt=("forward", "pass_same", "info"), ops_abs=("inverse", "pass_mixed", "info"))
    # two bad events of different kinds, in both orders; the time break sits on unit 0, whose first event is at 10
    for k, (name, i_time, i_oop) in enumerate((("time_then_oop", 150, 260), ("oop_then_time", 260, 150))):
        for meta in (gray, rgb):
            ev = stream(20 + k, meta)
            place(ev, meta, i_time, 0)
            out += pair(f"err_{name}_{meta['channels']}ch", "errors", meta, ev, (0, n1, n),
                        (br(i_time, "time"), br(i_oop, "oop")), ops_dt=("forward", "info"), ops_abs=("inverse", "info"))
    # two time breaks in different units: the one LATER in the input sits in unit 0, whose run is first in sorted order,
    # so the forward chain meets it (and lowers the limit to 270) while unit 1's, at 140, is the batch's bad event;
    # every other unit has by then written its times past 140
    for meta in (gray, rgb):
        ev = stream(30, meta)
        place(ev, meta, 270, 0)
        place(ev, meta, 140, 1)
        out += pair(f"err_two_times_{meta['channels']}ch", "errors", meta, ev, (0, n1, n),
                    (br(140, "time"), br(270, "time")), ops_dt=("forward", "info"), ops_abs=("inverse", "info"),
                    facts=dict(bad_unit=1, later_unit=0))
    # the channel byte: None in a three-channel plane is channel 0; c = 3 in RGB and c = 1 in gray are outside
    ev = stream(40, rgb)
    none0 = np.flatnonzero(ev["c"] == 0)[::2]
    ev["c"][none0] = NONE
    out += pair("err_c_none_is_channel_0_3ch", "errors", rgb, ev, (0, n1, n), (),
                ops_dt=("forward", "info"), ops_abs=("inverse", "info"), facts=dict(none=len(none0)))
    out += pair("err_c_3_in_rgb", "errors", rgb, stream(41, rgb), (0, n1, n), (br(130, "c", 3),),
                ops_dt=("forward", "info"), ops_abs=("inverse", "info"))
    out += pair("err_c_1_in_gray", "errors", gray, stream(42, gray), (0, n1, n), (br(130, "c", 1),),
                ops_dt=("forward", "info"), ops_abs=("inverse", "info"))
    return out


# ---- time edges -----------------------------------------------------------------------------------------------------

TIME_REFS = (1, 255, 5000, 1 << 31, U32)


def round_up(t, ref):
    return t if t % ref == 0 else (t // ref + 1) * ref


def time_cases():
    """Plane 2x1: unit 0 carries the edge, unit 1 runs beside it.  Each stream once in one batch and once cut between
    the two events concerned."""
    out = []
    A = 1000

    def ev_of(rows):  # (unit, t)
        m = meta_of(2, 1, 1)
        return from_units(m, [r[0] for r in rows], 5, [r[1] for r in rows], 0xBEEF)

    def both_cuts(name, meta, ev, cut, breaks, ops, facts, tail_bad=False):
        """+ a last batch of one event per unit: the state.  Unit 0's has t = 0 (DeltaT) or 2^32 - 1 (AbsoluteT), which
        is bad only where the unit's time stands past 2^32 - 1 (tail_bad)."""
        res, n0 = [], len(ev)
        ev = np.concatenate([ev, ev_of([(0, U32 if meta["time_mode"] == 1 else 0), (1, U32 if meta["time_mode"] == 1 else 11)])])
        if tail_bad:
            breaks = breaks + (br(n0, "timebad", ops=(ops[0],)),)
        for how, cuts in (("whole", (0, n0, n0 + 2)), ("cut", (0, cut, n0, n0 + 2))):
            _, body = apply_breaks(meta, ev, (), False)
            res.append(case(f"{name}/{how}", "time", meta, ops, cuts, events=ev, body=body, breaks=breaks,
                            facts=dict(facts, cut=cut)))
        return res

    for ref in TIME_REFS:
        for cam, version in ((0, 2), (DVS_CAM, 2), (0, 0)):
            tagname = f"ref{ref}_cam{cam}_v{version}"
            rounds_f = cam == 0 and version > 0
            up = (lambda t: round_up(t, ref)) if rounds_f else (lambda t: t)
            meta = meta_of(2, 1, 1, version=version, ref=ref, cam=cam)
            T1 = up(A)
            # forward: T + t = 2^32 - 1 exactly; then t = 0 (fine unless the round-up of 2^32 - 1 passed it); then 1
            over = up(U32) > U32
            ev = ev_of([(0, A), (1, 0), (0, U32 - T1), (1, 0), (0, 0), (0, 1), (1, 0)])
            out += both_cuts(f"time_fwd_sum_max_{tagname}", meta, ev, 2,
                             (br(4 if over else 5, "timebad", ops=("forward",)),), ("forward", "info"),
                             dict(t_out={2: U32}, round_past_u32=over), tail_bad=over)
            ev = ev_of([(0, A), (1, 0), (0, U32 - T1 + 1), (1, 0), (0, 0)])
            out += both_cuts(f"time_fwd_sum_2p32_{tagname}", meta, ev, 2, (br(2, "timebad", ops=("forward",)),),
                             ("forward", "info"), dict(sum=1 << 32))
            if version == 0:
                continue  # a v0 stream is DeltaT: no inverse, no AbsoluteT info
            meta = meta_of(2, 1, 1, version=version, time_mode=1, ref=ref, cam=cam)
            rounds_i = cam == 0
            L = round_up(A, ref) if rounds_i else A
            ev = ev_of([(0, A), (1, 0), (0, L), (1, 0), (0, L)])  # t = L: dt = 0 (twice where L is on the grid)
            bad = () if round_up(L, ref) == L or not rounds_i else (br(4, "timebad", ops=("inverse",)),)
            out += both_cuts(f"time_inv_t_eq_L_{tagname}", meta, ev, 2, bad, ("inverse", "info"), dict(L=L))
            if L <= U32:
                ev = ev_of([(0, A), (1, 0), (0, L - 1), (1, 0), (0, L)])
                ops = ("inverse",) if L - 1 >= A else ("inverse", "info")  # the raw time is A: info minds t < A only
                out += both_cuts(f"time_inv_t_eq_L_minus_1_{tagname}", meta, ev, 2, (br(2, "timebad", ops=ops),),
                                 ("inverse", "info"), dict(L=L, between=A < L - 1 < L))
            if rounds_i and L - A > 1 and L <= U32:  # strictly between the raw time and its round-up
                mid = A + (L - A) // 2
                ev = ev_of([(0, A), (1, 0), (0, mid), (1, 0), (0, round_up(mid, ref))])
                out += both_cuts(f"time_inv_between_{tagname}", meta, ev, 2, (br(2, "timebad", ops=("inverse",)),),
                                 ("inverse", "info"), dict(L=L, mid=mid))
            # L rounded past u32: the unit's next event is the bad one even at t = 2^32 - 1
            big = U32 - 3
            Lb = round_up(big, ref) if rounds_i else big
            ev = ev_of([(0, big), (1, 0), (0, U32), (1, 0), (0, U32)])
            bad = (br(2, "timebad", ops=("inverse",)),) if Lb > U32 else ()
            out += both_cuts(f"time_inv_L_past_u32_{tagname}", meta, ev, 2, bad, ("inverse", "info"),
                             dict(L=Lb, past=Lb > U32), tail_bad=Lb > U32)
    return out


# ---- fold arms ------------------------------------------------------------------------------------------------------

def absolute_raw(meta, units, dts):
    """AbsoluteT times whose differences to the unit's previous RAW time are dts (what adder-info takes back)"""
    last, t = {}, []
    for u, dt in zip(units.tolist(), dts.tolist()):
        last[u] = last.get(u, 0) + dt
        t.append(last[u])
    assert max(t) <= U32
    return np.array(t, np.int64)


FOLD12 = ((0, 3, 4, "lower"), (0, 255, 9, "ignored"), (0, 3, 2, "offered_and_raises"),
          (0, 3, 4, "offered_and_does_not"),  # a == min
          (0, 2, 1, "offered_and_does_not"),  # a == max
          (0, 128, 0, "replace_by_inf"), (0, 0, 4, "lower"), (0, 128, 2, "replace_by_128"),
          (1, 127, 1, "offered_and_raises"), (0, 200, 7, "to_zero"), (0, 128, 3, "sticky"),
          (2, 0, U32, "offered_and_does_not"))  # (unit, d, relative time, the arm it takes)


def fold_cases():
    out = []
    for absolute in (False, True):
        meta = meta_of(4, 4, 1, time_mode=1 if absolute else 0)
        word = "abs" if absolute else "dt"
        # 6 000 events: units 0..9 ordinary; units 10..15 each hold one event with an extreme time
        rng = np.random.default_rng([16, int(absolute)])
        n = 6000
        units = rng.integers(0, 10, n)
        d = rng.choice(np.array([3, 4, 5, 6, 7, 8, 9, 10, 255], np.uint8), n)
        dt = rng.integers(8, 3000, n)
        # (unit, d, relative time); units 11..13 hold nothing else, so that a relative time of 2^32 - 1 fits AbsoluteT
        special = {0: (0, 128, 0),  # min = +inf at the batch's first position
                   700: (7, 126, 1), 701: (8, 126, 1),  # raises max; a == max
                   900: (11, 0, U32), 901: (12, 0, U32),  # lowers min as far as an event can; a == min
                   1500: (0, 128, 0), 1501: (1, 9, 2), 2000: (2, 128, 5), 2001: (3, 0, 2999),
                   4500: (4, 200, 3),  # the sticky zero, tiles of the scan on both sides
                   4600: (9, 127, 1), 4700: (13, 0, U32), 4800: (5, 128, 4), 4801: (6, 250, 1),
                   5999: (7, 127, 0)}  # a == max at the batch's last position
        sp = np.array(sorted(special))
        dup = rng.integers(1, n, 600)  # equal intensities: the event before, again
        dup = dup[~np.isin(dup, sp) & ~np.isin(dup - 1, sp)]
        d[dup], dt[dup] = d[dup - 1], dt[dup - 1]
        for i, (u, dd, tt) in special.items():
            units[i], d[i], dt[i] = u, dd, tt
        t = absolute_raw(meta, units, dt) if absolute else dt
        ev = from_units(meta, units, d, t, rng.integers(0, 1 << 16, n))
        out.append(case(f"fold_6000/{word}", "fold", meta, ("info",), (0, n), events=ev,
                        facts=dict(special={i: s for i, s in special.items()}, zero_at=4500)))
        # the 12 events that hold each arm once, whole and cut at every position
        units = np.array([r[0] for r in FOLD12])
        d, dt = np.array([r[1] for r in FOLD12]), np.array([r[2] for r in FOLD12], np.int64)
        t = absolute_raw(meta, units, dt) if absolute else dt
        ev = from_units(meta, units, d, t, 0x1234)
        for k in range(0, 12):
            cuts = (0, 12) if k == 0 else (0, k, 12)
            out.append(case(f"fold_12_cut{k}/{word}", "fold", meta, ("info",), cuts, events=ev,
                            facts=dict(arms=tuple(r[3] for r in FOLD12))))
    return out


def fold_census(c):
    """-> (the arms the oracle took on the case's events, the oracle)"""
    arms = []
    r = R.Info(c["meta"], census=arms)
    assert r.run(c["events"]) is None
    return arms, r


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        cases = tag_cases() + unit_cases() + grid_cases() + error_cases() + time_cases() + fold_cases()
        assert len({c["name"] for c in cases}) == len(cases)
        _CASES = {c["name"]: c for c in cases}
    return _CASES


def names(group=None):
    return [n for n, c in all_cases().items() if group is None or c["group"] == group]
