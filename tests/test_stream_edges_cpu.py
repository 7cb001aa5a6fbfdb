"""The census of tests/stream_edge_cases.py, without a GPU: every case reaches what it was built for -- positions,
counts, the index the restatement reports as bad, the arms the fold took -- and the inputs of the older random streams
(test_gpu_stream_tools.random_stream) reach none of it, which is why the cases exist.  Also the tag-aware record codec
of adder_stream_np.py against its older reader and writer."""
import struct

import numpy as np
import pytest

import adder_stream_np as S
import stream_edge_cases as E
import stream_tools_oracle as R

CASES = E.all_cases()
U32 = E.U32


def sources(c):
    return ("wire",) if c["events"] is None else ("events", "wire")


@pytest.mark.parametrize("name", E.names())
def test_the_restatement_stops_where_the_case_claims(name):
    """bad index and records consumed, batch by batch: claimed from the breaks, scanned from the bytes, and what the
    oracle says -- for every op and both sources"""
    c = CASES[name]
    for source in sources(c):
        scan = E.scanned(c, source)
        for op in c["ops"]:
            want = E.claimed(c, op, source)
            got = E.expected(c, op, source)
            assert [(r["bad"], r["consumed"]) for r in got] == want, (source, op)
            for (oop, end), (bad, consumed) in zip(scan, want):
                assert end == consumed and (oop is None or (bad is not None and bad <= oop)), (source, op)
                if bad is not None and not any(b["kind"] in ("time", "timebad") for b in c["breaks"]):
                    assert bad == oop
            for r in got:
                assert r["done"] == (r["consumed"] if r["bad"] is None else r["bad"]) <= r["consumed"] <= r["n"]
                if op != "info":
                    assert len(r["out"]) == r["done"] * (12 if source == "events" else c["record_bytes"])


def test_case_limits():
    for c in CASES.values():
        assert c["n"] <= 10_000 and c["meta"]["width"] <= 32 and c["meta"]["height"] <= 32
        if c["group"] != "units":
            assert c["meta"]["width"] <= 16 and c["meta"]["height"] <= 16
    groups = {c["group"] for c in CASES.values()}
    assert groups == {"tags", "units", "grid", "errors", "time", "fold"}


@pytest.mark.parametrize("name", E.names("tags"))
def test_tag_cases(name):
    c = CASES[name]
    assert c["events"] is None and c["meta"]["channels"] == 3
    ev, tag, spare, end = S.decode_records(c["body"], 3)
    b = np.frombuffer(c["body"], np.uint8).reshape(-1, 11)
    first = min([br["i"] for br in c["breaks"]], default=c["n"])
    assert end == first
    live = np.ones(c["n"], bool)
    live[[br["i"] for br in c["breaks"]]] = False
    zero, one = live & (tag == 0), live & (tag == 1)
    assert c["facts"]["tag0"] - len(c["breaks"]) <= zero.sum() <= c["facts"]["tag0"] and zero.sum() > 100 and one.sum() > 100 and (zero | one)[live].all()
    assert (b[zero, 10] != 0).all() and len(set(b[zero, 10].tolist())) > 50  # the byte behind t of a None record
    assert zero[:first].sum() > 50 and (ev["c"][zero] == 0xFF).all()
    kinds = [(br["kind"], br["arg"]) for br in sorted(c["breaks"], key=lambda br: br["i"])]
    want = {"tags_mixed": [], "tags_end_tag2": [("tag", 2)], "tags_end_tag255": [("tag", 255)],
            "tags_tag9_then_eof": [("tag", 9), ("eof", None)], "tags_eof_then_tag7": [("eof", None), ("tag", 7)]}
    assert kinds == want[name.split("/")[0]]
    for br in c["breaks"]:
        r = b[br["i"]]
        if br["kind"] == "tag":
            assert r[4] == br["arg"] > 1 and not (r[:4] == 255).all()
        else:
            assert (r[:4] == 255).all() and r[4] <= 1
    # records that look valid lie behind every end
    assert all(live[br["i"] + 1] and E.unit_of(c["meta"], ev[br["i"] + 1:br["i"] + 2])[0] >= 0 for br in c["breaks"])
    assert set(c["ops"]) >= {"pass_same", "pass_mixed", "info"} and ("forward" in c["ops"]) != ("inverse" in c["ops"])


@pytest.mark.parametrize("name", E.names("units"))
def test_unit_count_cases(name):
    c = CASES[name]
    meta, units = c["meta"], E.n_units(c["meta"])
    assert (meta["width"], meta["height"], meta["channels"]) in E.UNIT_PLANES
    p_oop, p_eof = c["facts"]["p_oop"], c["facts"]["p_eof"]
    ev, _, _, end = S.decode_records(c["body"], meta["channels"])
    u = E.unit_of(meta, ev)
    assert end == p_eof and u[p_oop] == -1 and (u[[p_oop - 1, p_oop + 1, p_eof - 1, p_eof + 1]] == 0).all()
    assert (u[p_eof + 1:] >= 0).all() and len(u) - p_eof > 100  # valid-looking records behind the EOF
    a, b = c["cuts"][:2]
    assert a <= p_oop < b <= p_eof  # each sentinel in a batch of its own, unit 0 around it in that batch
    for batch in (0, 1):
        k = E.sorted_keys(c, batch)
        assert k[-1] == units and k[0] == 0 and (k == units - 1).sum() >= batch  # sentinel behind the last unit
    if (meta["width"], meta["height"]) == (8, 8):  # a three-channel event in a gray plane
        assert c["events"]["c"][p_oop] == 2 and c["events"]["x"][p_oop] < 8 and ev["x"][p_oop] == 8
    assert {E.n_units(CASES[n]["meta"]) for n in E.names("units")} == {1, 255, 256, 64, 1024}


@pytest.mark.parametrize("name", E.names("grid"))
def test_grid_cases(name):
    c = CASES[name]
    n, hist = c["facts"]["n"], c["facts"]["histogram"]
    assert c["cuts"] == (0, n, n + E.FOLLOW)
    k = E.sorted_keys(c)
    assert np.array_equal(k, hist) and len(k) == n
    head = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    length = np.diff(np.concatenate([head, [n]]))
    runs = dict(zip(head.tolist(), length.tolist()))
    if "span" in name:
        assert runs[200] == 601 and 200 + 601 - 1 == 800 and all(runs[p] == 1 for p in range(801, n))
    else:
        assert runs[n - 1] == 1 or n == 1
        for p in (256, 512):
            assert p in runs or p >= n
        if n > 256:
            assert runs[255] == 1
        if n == 1025:
            assert runs == {0: 255, 255: 1, 256: 256, 512: 512, 1024: 1}
    # the input is not in sorted order (but for the smallest)
    u = E.unit_of(c["meta"], c["events"][:n])
    assert n <= 2 or not np.array_equal(u, k)
    assert {CASES[x]["facts"]["n"] for x in E.names("grid")} == set(E.GRID_N)


def test_error_cases_cover_the_interplay():
    names = {n.rsplit("/", 1)[0] for n in E.names("errors")}
    for stem in ("bad_at_0", "bad_at_last", "eof_at_0", "eof_at_last", "eof_then_bad", "bad_then_eof", "time_then_oop",
                 "oop_then_time", "two_times"):
        assert {f"err_{stem}_1ch", f"err_{stem}_3ch"} <= names
    for n in E.names("errors"):
        c = CASES[n]
        assert c["cuts"] == (0, 300, 400) and c["events"] is not None
        ops = set(c["ops"])
        assert "info" in ops and (("forward" in ops) if n.endswith("/dt") else ("inverse" in ops))
    c = CASES["err_bad_at_0_1ch/dt"]
    assert E.claimed(c, "forward", "events")[0] == (0, 300) and E.expected(c, "forward", "wire")[0]["done"] == 0
    c = CASES["err_eof_at_last_3ch/abs"]
    assert E.claimed(c, "inverse", "wire")[0] == (None, 299) and E.claimed(c, "inverse", "events")[0] == (299, 300)
    assert c["events"]["x"][299] == c["events"]["y"][299] == 0xFFFF  # an AdderEvent has no EOF: outside the plane
    assert E.claimed(CASES["err_eof_then_bad_1ch/dt"], "forward", "wire")[0] == (None, 100)
    assert E.claimed(CASES["err_bad_then_eof_1ch/dt"], "forward", "wire")[0] == (100, 200)
    # two kinds: the time break is an overflow (forward) or a time below the previous one (inverse, AbsoluteT info)
    for ch in (1, 3):
        for word, op in (("dt", "forward"), ("abs", "inverse"), ("abs", "info")):
            assert E.claimed(CASES[f"err_time_then_oop_{ch}ch/{word}"], op, "events")[0][0] == 150
            assert E.claimed(CASES[f"err_oop_then_time_{ch}ch/{word}"], op, "events")[0][0] == 150
            assert E.claimed(CASES[f"err_two_times_{ch}ch/{word}"], op, "events")[0][0] == 140
        assert E.claimed(CASES[f"err_time_then_oop_{ch}ch/dt"], "info", "events")[0][0] == 260
        # the overflow that is NOT the bad event sits later in the input and in the unit whose run is walked first,
        # and units other than these two have events between the two indices: their times are worked out past 140
        c = CASES[f"err_two_times_{ch}ch/dt"]
        u = E.unit_of(c["meta"], c["events"])
        assert (u[140], u[270]) == (1, 0) and c["events"]["t"][140] == c["events"]["t"][270] == U32
        assert (u[141:270] > 1).sum() > 100
        r = R.Migration(c["meta"], R.ABSOLUTE_T)
        assert r.run(np.delete(c["events"][:300], 140))[1] == 269  # with 140 left out the other one is bad
    c = CASES["err_c_none_is_channel_0_3ch/dt"]
    assert (c["events"]["c"] == 0xFF).sum() == c["facts"]["none"] > 20 and E.claimed(c, "forward", "events")[0][0] is None
    assert (S.decode_records(c["body"], 3)[1] == 0).sum() == c["facts"]["none"]
    assert E.claimed(CASES["err_c_3_in_rgb/dt"], "forward", "wire")[0][0] == 130
    assert E.claimed(CASES["err_c_1_in_gray/dt"], "forward", "events")[0][0] == 130
    assert E.claimed(CASES["err_c_1_in_gray/dt"], "forward", "wire")[0][0] is None  # a 9-byte record has no c


@pytest.mark.parametrize("name", E.names("time"))
def test_time_cases(name):
    c = CASES[name]
    f, meta, ev = c["facts"], c["meta"], c["events"]
    assert meta["ref_interval"] in E.TIME_REFS and len(c["cuts"]) in (3, 4)
    if "/cut" in name:
        assert c["cuts"][1] == f["cut"] == 2  # between unit 0's first event (0) and its second (2)
    op = c["ops"][0]
    res = E.expected(c, op, "events")
    flat_bad = [c["cuts"][k] + r["bad"] for k, r in enumerate(res) if r["bad"] is not None]
    out = b"".join(r["out"] for r in res)
    t_of = {}
    pos = 0
    for k, r in enumerate(res):
        got = np.frombuffer(r["out"], S.EVENT_DTYPE)
        for j in range(r["done"]):
            t_of[c["cuts"][k] + j] = int(got["t"][j])
    if "fwd_sum_max" in name:
        assert t_of[2] == U32 and f["t_out"] == {2: U32}
        rounds = meta["source_camera"] == 0 and meta["version"] > 0
        assert f["round_past_u32"] == (rounds and U32 % meta["ref_interval"] != 0)
        assert flat_bad[0] == (4 if f["round_past_u32"] else 5)
        if not f["round_past_u32"]:
            assert t_of[4] == U32  # t = 0 on top of 2^32 - 1
    elif "fwd_sum_2p32" in name:
        assert flat_bad == [2] and 2 not in t_of
    elif "inv_t_eq_L/" in name.replace("_ref", "/ref"):
        assert flat_bad == [] and t_of[0] == 1000 and int(ev["t"][2]) == f["L"] and t_of[2] == 0 and t_of[4] == 0
    elif "L_minus_1" in name:
        assert flat_bad == [2] and int(ev["t"][2]) == f["L"] - 1
        info_bad = [r["bad"] for r in E.expected(c, "info", "events")]
        assert any(b is not None for b in info_bad) == (f["L"] - 1 < 1000)
    elif "between" in name:
        assert 1000 < f["mid"] < f["L"] and flat_bad == [2]
        assert all(r["bad"] is None for r in E.expected(c, "info", "events"))  # adder-info takes the raw time
    elif "L_past_u32" in name:
        assert f["past"] == (f["L"] > U32) and (flat_bad[:1] == [2]) == f["past"]
        if not f["past"]:
            assert t_of[2] == U32 - f["L"] and t_of[4] == 0
    else:
        raise AssertionError(name)


def test_time_cases_cover_refs_cameras_and_version_0():
    names = E.names("time")
    for ref in E.TIME_REFS:
        for tail in ("cam0_v2", "cam6_v2", "cam0_v0"):
            for how in ("whole", "cut"):
                assert f"time_fwd_sum_max_ref{ref}_{tail}/{how}" in names
                assert f"time_fwd_sum_2p32_ref{ref}_{tail}/{how}" in names
        for tail in ("cam0_v2", "cam6_v2"):
            for stem in ("t_eq_L", "t_eq_L_minus_1", "L_past_u32"):
                assert f"time_inv_{stem}_ref{ref}_{tail}/cut" in names
        if ref > 1:
            assert f"time_inv_between_ref{ref}_cam0_v2/whole" in names
    assert CASES[f"time_inv_L_past_u32_ref5000_cam0_v2/whole"]["facts"]["past"]
    assert CASES[f"time_fwd_sum_max_ref{1 << 31}_cam0_v2/whole"]["facts"]["round_past_u32"]
    assert not CASES[f"time_fwd_sum_max_ref{U32}_cam0_v2/whole"]["facts"]["round_past_u32"]
    assert any(int(CASES[n]["events"]["t"].max()) == U32 for n in names)


@pytest.mark.parametrize("word", ["dt", "abs"])
def test_fold_cases_take_every_arm(word):
    c = CASES[f"fold_6000/{word}"]
    arms, r = E.fold_census(c)
    plain = R.Info(c["meta"])
    assert plain.run(c["events"]) is None
    assert (struct.pack("<3d", plain.min, plain.max, plain.count) ==
            struct.pack("<3d", r.min, r.max, r.count))  # the census changes nothing
    assert len(arms) == c["n"] == 6000 and set(arms) == set(R.FOLD_ARMS)
    zero = c["facts"]["zero_at"]
    assert zero >= E.SCAN_SPAN and arms[zero] == "to_zero" and arms.index("to_zero") == zero
    want = {0: "replace_by_inf", 700: "offered_and_raises", 701: "offered_and_does_not", 900: "lower",
            901: "offered_and_does_not", 1500: "replace_by_inf", 1501: "lower", 2000: "replace_by_128", 2001: "lower",
            4600: "offered_and_raises", 4700: "offered_and_does_not", 4800: "sticky", 4801: "sticky",
            5999: "offered_and_does_not"}
    assert {i: arms[i] for i in want} == want
    d = c["events"]["d"]
    assert ((d > 128) & (d < 255)).sum() == 2 and (d[:zero] == 128).sum() >= 3 and r.min == 0.0 and r.max == 2.0 ** 127
    before, after = set(arms[:zero]), set(arms[zero + 1:])
    assert before == set(R.FOLD_ARMS) - {"to_zero", "sticky"}
    assert after == {"ignored", "sticky", "offered_and_raises", "offered_and_does_not"}
    assert arms[:zero].count("lower") >= 5 and arms[:zero].count("offered_and_raises") >= 5
    for k in range(12):
        c = CASES[f"fold_12_cut{k}/{word}"]
        arms, _ = E.fold_census(c)
        assert tuple(arms) == c["facts"]["arms"] and set(arms) == set(R.FOLD_ARMS)
        assert c["cuts"] == ((0, 12) if k == 0 else (0, k, 12))
    # the carried min over the cuts: f64::MAX, +inf and 0.0 among them
    carried = set()
    for k in range(1, 12):
        r = R.Info(c["meta"])
        r.run(c["events"][:k])
        carried.add(r.min)
    assert {float("inf"), 0.0, 2.0, 0.25, 0.5} <= carried


def test_the_older_random_streams_reach_none_of_this():
    """what test_gpu_stream_tools.random_stream draws: no d in 129..254, only Some(c) records, no sum within 1 000
    ticks of 2^32 -- the reason for stream_edge_cases.py, kept on record"""
    import test_gpu_stream_tools as G
    for seed, ch, absolute in ((1, 1, False), (2, 3, False), (3, 3, True), (4, 1, True)):
        rng = np.random.default_rng(seed)
        ev = G.random_stream(rng, 9000, 7, 5, ch, absolute, big_t=True)
        d = ev["d"]
        assert not ((d > 128) & (d < 255)).any()
        meta = dict(width=7, height=5, channels=ch, version=2, time_mode=int(absolute), ref_interval=255,
                    source_camera=0, tps=1, delta_t_max=1, adu_interval=0)
        body = S.write_adder(meta, ev, close=False)[len(S.build_header(meta)):]
        if ch == 3:
            assert (np.frombuffer(body, np.uint8).reshape(-1, 11)[:, 4] == 1).all()
        out, bad = R.Migration(dict(meta, time_mode=0), R.ABSOLUTE_T).run(ev) if not absolute else (
            [tuple(int(v) for v in (e["x"], e["y"], e["c"], e["d"], e["t"])) for e in ev], None)
        assert bad is None and max(o[4] for o in out) < (1 << 32) - 1000
        arms = []
        R.Info(meta, census=arms).run(ev)
        assert "to_zero" not in arms and "sticky" not in arms


def test_tag_aware_codec_equals_the_older_one_on_some_records():
    rng = np.random.default_rng(8)
    for ch in (1, 3):
        meta = E.meta_of(9, 7, ch)
        ev = E.random_events(rng, meta, 500)
        ev["pad"] = 0
        ev["t"][:4] = [0, 1, U32, 0x01020304]
        hdr = len(S.build_header(meta))
        body = S.write_adder(meta, ev, close=False)[hdr:]
        assert S.encode_records(ev, ch, np.ones(500, np.uint8), np.zeros(500, np.uint8)) == body
        got, tag, spare, end = S.decode_records(body, ch)
        _, want, closed = S.read_adder(S.write_adder(meta, ev))
        assert end == 500 and np.array_equal(got, want) and closed and (tag == 1).all() and (spare == 0).all()
        got, _, _, end = S.decode_records(body + S.EOF, ch)
        assert end == 500  # the EOF record ends both readers at the same place
    # a None record: d at byte 5, t at bytes 6..9, byte 10 carried
    rec = bytes([0, 3, 0, 2, 0, 77, 1, 2, 3, 4, 0x5A])
    ev, tag, spare, end = S.decode_records(rec, 3)
    assert (int(ev["x"][0]), int(ev["y"][0]), int(ev["c"][0]), int(ev["d"][0]), int(ev["t"][0])) == \
        (3, 2, 0xFF, 77, 0x01020304)
    assert (tag[0], spare[0], end) == (0, 0x5A, 1) and S.encode_records(ev, 3, tag, spare) == rec
    assert S.decode_records(bytes([0, 3, 0, 2, 2]) + bytes(6), 3)[3] == 0  # tag > 1 ends the stream
    assert S.decode_records(S.EOF, 3)[3] == 0
