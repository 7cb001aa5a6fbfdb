"""csrc/adder_compressed_logic.hpp -- the text adder_compressed_model.hip compiles -- run serially by g++
(tests/cpu_sim/compressed_model_main.cpp) against the host sink: the symbols it emits, fed to
CompressedEncoder.ingest_symbols, must give the bytes CompressedEncoder.ingest gives for the same events, and its
reconstructed events must be what compressed_decode returns.  Integer- and bit-exact throughout.  No GPU needed."""
import subprocess

import numpy as np
import pytest

import adder_amd as A
import compressed_model_cases as CM
from oracle import compressed_oracle as CO

CASES = CM.cpu_cases()


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return CM.build_sim(tmp_path_factory.mktemp("compressed_model_sim"))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_symbols_give_the_host_sinks_bytes_and_events(case, sim, tmp_path):
    ev = case["events"]()
    want = CM.host_stream(case, ev, threads=1)
    got = CM.run_sim(sim, case, ev, tmp_path)
    for threads in (1, 4):
        assert CM.symbol_stream(case, got["symbols"], threads=threads) == want, threads
    dec = CM.decode(case, want)
    recon = np.concatenate(got["events"]) if got["events"] else np.zeros(0, A.EVENT_DTYPE)
    assert np.array_equal(recon, dec)
    assert got["events_in"] == len(ev) and got["dropped"] == len(ev) - len(dec)
    assert sum(got["bitshift"]) == len(dec)
    if case["cmax"] == 0:  # never shifts
        assert sum(got["bitshift"][1:15]) == 0
    # the blocked cut walk at other widths (checked against the serial rule inside the program)
    for lanes in (1, 3):
        again = CM.run_sim(sim, case, ev, tmp_path, cut_lanes=lanes)
        assert all(np.array_equal(a, b) for a, b in zip(again["symbols"], got["symbols"]))


def test_cut_walk_equals_the_serial_rule_exhaustively(sim):
    assert subprocess.call([sim, "cuts"]) == 0


def test_symbol_counts_are_64_bit(sim):
    assert subprocess.call([sim, "sizes"]) == 0


def test_ingest_symbols_refusals(sim, tmp_path):
    case = next(c for c in CASES if c["name"] == "arms")
    ev = case["events"]()
    adus = CM.run_sim(sim, case, ev, tmp_path)["symbols"]
    assert len(adus) >= 2
    # mixed use, both ways
    enc = CM.encoder_for(case)
    enc.ingest(ev[:3])
    with pytest.raises(A.AdderHipError):
        enc.ingest_symbols(adus[0])
    enc.destroy()
    enc = CM.encoder_for(case)
    enc.ingest_symbols(adus[0])
    with pytest.raises(A.AdderHipError):
        enc.ingest(ev[:3])
    # the refusals below leave the encoder as it was: the rest of the stream still goes in, and gives the same bytes
    bad = adus[1].copy()
    bad[7] = 4 << 10                         # an unknown context
    with pytest.raises(A.AdderHipError):
        enc.ingest_symbols(bad)
    for ctx, entries in ((0, 514), (1, 257), (2, 17), (3, 2)):
        bad = adus[1].copy()
        bad[7] = ctx << 10 | entries         # an index outside its context's table
        with pytest.raises(A.AdderHipError):
            enc.ingest_symbols(bad)
    with pytest.raises(A.AdderHipError):
        enc.ingest_symbols(adus[1][:-1])     # no eof
    bad = adus[1].copy()
    bad[9] = 3 << 10                         # an eof before the end
    with pytest.raises(A.AdderHipError):
        enc.ingest_symbols(bad)
    with pytest.raises(A.AdderHipError):
        enc.ingest_symbols(adus[0])          # the ADU that starts at 0 again: not the encoder's next
    with pytest.raises(A.AdderHipError):
        enc.ingest_symbols(np.zeros(0, np.uint16))
    for s in adus[1:]:
        enc.ingest_symbols(s)
    out = enc.close()
    enc.destroy()
    assert out == CM.host_stream(case, ev)


# ---------------------------------------------------------------- census
class Census:
    """Counts, on the oracle's restatement of the reference (its coder switched off), the arms the cases reach."""

    def __init__(self, monkeypatch):
        self.n = {}
        c = self
        ctx = CO.Contexts
        orig_rtb, orig_rtb2 = ctx.residual_to_bitshift, ctx.residual_to_bitshift2
        orig_eti, orig_pred = ctx.event_to_intensity, CO.generate_t_prediction
        orig_ingest, orig_compress = CO.EventCube.ingest_event, CO.EventAdu.compress
        orig_out_ingest = CO.CompressedOutput.ingest_event

        def rtb(self, r):
            c.hit("intra_full" if abs(r) >= 127 else "intra_short")
            if r < 0:
                c.hit("intra_negative")
            return orig_rtb(self, r)

        def rtb2(self, t_prediction, r, event, prev, dt_ref, c_thresh_max):
            bs, res = orig_rtb2(self, t_prediction, r, event, prev, dt_ref, c_thresh_max)
            c.hit(f"inter_bitshift_{bs}")
            tres = abs(r)  # the loop once more, for the `recon_t < prev.t` break
            if tres >= 127:
                actual = orig_eti(event[0], max(event[1] - prev[1], 0), dt_ref)
                recon = actual
                halvings = 0
                while tres > 127 and actual - c_thresh_max < recon and actual + c_thresh_max > recon:
                    tres >>= 1
                    halvings += 1
                    c.hit(f"halvings_{min(halvings, 15)}")
                    rt = (t_prediction + tres) & 0xFFFFFFFF
                    if rt < prev[1]:
                        c.hit("recon_before_prev_break")
                        break
                    recon = orig_eti(event[0], rt - prev[1], dt_ref)
            if bs == 15:
                t = (t_prediction + res) & 0xFFFFFFFF
            else:
                t = (t_prediction + (CO._wrap_i16(res) << bs)) & 0xFFFFFFFF
            if t < prev[1]:
                c.hit("clamp_to_prev")
            return bs, res

        def eti(d, delta_t, dt_ref):
            c.hit("d_128" if d == 128 else "d_ge_129" if d >= 129 else "d_table")
            if delta_t == 0:
                c.hit("delta_t_0")
            return orig_eti(d, delta_t, dt_ref)

        def pred(idx, d_residual, last_delta_t, prev, num_intervals, dt_ref, start_t):
            if idx > 1:
                if abs(d_residual) > 14:
                    c.hit("d_residual_beyond_14")
                if prev[0] == 255:
                    c.hit("prev_d_255")
            return orig_pred(idx, d_residual, last_delta_t, prev, num_intervals, dt_ref, start_t)

        def ingest(self, x, y, ch, d, t):
            px = self.lists[ch][y - self.start_y][x - self.start_x]
            if len(px) > 1 and t <= px[-1][1]:
                c.hit("dropped_third_or_later")
            if len(px) == 1 and t <= px[0][1]:
                c.hit("kept_second_not_later")
            return orig_ingest(self, x, y, ch, d, t)

        def compress(self, c_thresh_max):
            skips = [cube.skip_cube for cube in self.all_cubes()]
            if all(skips):
                c.hit("empty_adu")
            hit = [i for i, s in enumerate(skips) if not s]
            if hit and any(skips[hit[0]:hit[-1]]):
                c.hit("skipped_cube_between")
            c.cut_run += 1
            return orig_compress(self, c_thresh_max)

        def out_ingest(self, x, y, ch, d, t):
            before = c.n.get("adus", 0)
            orig_out_ingest(self, x, y, ch, d, t)
            if c.n.get("adus", 0) == before:
                c.cut_run = 0
            elif c.cut_run >= 10:
                c.hit("dense_cut_10_in_a_row")

        def compress_counted(self, c_thresh_max):
            c.hit("adus")
            return compress(self, c_thresh_max)

        self.cut_run = 0
        monkeypatch.setattr(ctx, "residual_to_bitshift", rtb)
        monkeypatch.setattr(ctx, "residual_to_bitshift2", rtb2)
        monkeypatch.setattr(ctx, "event_to_intensity", staticmethod(eti))
        monkeypatch.setattr(CO, "generate_t_prediction", pred)
        monkeypatch.setattr(CO.EventCube, "ingest_event", ingest)
        monkeypatch.setattr(CO.EventAdu, "compress", compress_counted)
        monkeypatch.setattr(CO.CompressedOutput, "ingest_event", out_ingest)
        monkeypatch.setattr(CO.ArithEncoder, "encode", lambda self, sym, out: None)  # the census needs no bytes

    def hit(self, arm):
        self.n[arm] = self.n.get(arm, 0) + 1


def test_the_cases_reach_every_arm(monkeypatch):
    census = Census(monkeypatch)
    cmax_seen = set()
    for case in CASES:
        if case["name"] == "virat_whole":
            continue  # (real data; the arms are counted on the built streams)
        ev = case["events"]()
        co = CO.CompressedOutput(case["w"], case["h"], case["c"], tps=case["tps"], ref_interval=case["ref"],
                                 delta_t_max=case["dtm"], adu_interval=case["adu"], c_thresh_max=case["cmax"],
                                 write_header=case["header"])
        for e in ev:
            co.ingest_event(int(e["x"]), int(e["y"]), int(e["c"]), int(e["d"]), int(e["t"]))
        co.close()
        cmax_seen.add(case["cmax"])
    n = census.n
    print(sorted(n.items()))
    for arm in ("intra_short", "intra_full", "intra_negative", "inter_bitshift_0", "inter_bitshift_15",
                "recon_before_prev_break", "clamp_to_prev", "d_128", "d_ge_129", "prev_d_255", "d_residual_beyond_14",
                "delta_t_0", "dropped_third_or_later", "kept_second_not_later", "empty_adu", "skipped_cube_between",
                "dense_cut_10_in_a_row"):
        assert n.get(arm, 0) > 0, arm
    # Bit shifts 1..14: the f64 loop halves the residual up to many times in these cases (every depth below is
    # reached), but the shift it settles on is one less than the halvings made, and at that shift the residual was
    # still above 127 -- so the reference's last test always falls back to the full form.  No input makes the host
    # encoder emit a shift in 1..14 (test_lossy_bit_shift_only_emits_0_and_15 sweeps the function for it); what can be
    # reached, and is asked for here, is the loop at several depths in 1..14 and its two exits.
    assert not [b for b in range(1, 15) if n.get(f"inter_bitshift_{b}", 0)]
    depths = [b for b in range(1, 15) if n.get(f"halvings_{b}", 0)]
    assert len(depths) >= 8, depths
    assert {0, 25} <= cmax_seen


def test_lossy_bit_shift_only_emits_0_and_15(sim):
    assert subprocess.call([sim, "shifts"]) == 0


def test_first_event_of_a_cube_before_start_t_is_negative_intra(sim, tmp_path):
    """An event earlier than its ADU's start_t, first of its cube: r < 0 against (d, start_t), the full form."""
    case = next(c for c in CASES if c["name"] == "arms_first_negative")
    got = CM.run_sim(sim, case, case["events"](), tmp_path)
    assert got["start_t"] == [0, 200, 400]   # one ADU per event at most: t = 1000 closes one, t = 1001 the next
    sym = got["symbols"][1]                  # start_t 200: events (1,1,t=1000), (2,2,t=5)

    def be64(words):
        r = 0
        for w in words:
            assert int(w) >> 10 == 1
            r = r << 8 | ((int(w) & 1023) - 1)
        return r - (1 << 64) if r >> 63 else r

    # 4 start_t bytes; pixel (1,1) is the cube's 18th: 17 no-events, then d, the full form, eight t bytes
    assert list(sym[4:4 + 17]) == [512] * 17 and sym[4 + 17] == 7 + 255 + 1 and sym[4 + 18] == (2 << 10 | 16)
    assert be64(sym[4 + 19:4 + 27]) == 1000 - 200
    k = 4 + 17 + 10 + 16                     # pixel (2,2): 16 more empty pixels after (1,1)'s ten symbols
    assert sym[k] == 0 + 255 + 1 and sym[k + 1] == (2 << 10 | 16)   # d residual 0; the full form
    assert be64(sym[k + 2:k + 10]) == 5 - 1000   # negative: earlier than the previous pixel's first event and start_t
