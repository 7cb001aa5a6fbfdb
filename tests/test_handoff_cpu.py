"""The numpy restatement of the stream hand-off kernels (handoff_oracle.py) against the independent implementations the
project already has -- the oracle's and the host library's raw sink, adder_amd.sharding on CPU tensors, the oracle's row
chunks -- and the properties by which the synthetic cases (handoff_cases.py) reach every edge of the kernels (the tile
carry, the pair walk, the block stride, every byte phase, two chunk workgroups).  Runs without a GPU."""
import numpy as np
import pytest

from oracle import oracle as O
import adder_amd as A
import handoff_cases as HC
import handoff_oracle as HO


def _i32(ev):
    import torch
    return torch.from_numpy(np.frombuffer(ev.tobytes(), np.int32).reshape(-1, 3).copy())


# ---- wire_bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("n", [0, 1, HC.WIRE_EVENTS - 1, HC.WIRE_EVENTS, HC.WIRE_EVENTS + 1])
def test_wire_bytes_equals_both_raw_sinks(channels, n):
    rec = 9 if channels == 1 else 11
    ev = HC.wire_events(n, channels)
    got = HO.wire_bytes(ev, rec).tobytes()
    assert len(got) == n * rec
    assert got == O.raw_events(ev, channels)
    assert got == A.raw_events(ev.astype(A.EVENT_DTYPE), channels)


@pytest.mark.parametrize("channels", [1, 3])
def test_wire_bytes_at_the_fields_extremes(channels):
    rec = 9 if channels == 1 else 11
    ev = HC.extreme_events(channels)
    assert ev["x"].max() == ev["y"].max() == 0xfffe and ev["t"].max() == 0xffffffff and ev["d"].max() == 255
    assert channels == 1 or (ev["c"] == 0).any()
    got = HO.wire_bytes(ev, rec).tobytes()
    assert got == O.raw_events(ev, channels) == A.raw_events(ev.astype(A.EVENT_DTYPE), channels)
    first = [0xff, 0xfe, 0xff, 0xfe] + ([] if channels == 1 else [1, 0]) + [255, 0xff, 0xff, 0xff, 0xff]
    assert list(got[:rec]) == first


def test_event_marks_round_trip():
    ev = HC.make_events(2, np.array([0, 255, 256, 21845, (1 << 22) - 1]), np.array([0, 1, 65536, (1 << 24) - 1, 5]))
    r, f, i = HC.source_of(ev)
    assert list(r) == [2] * 5 and list(f) == [0, 255, 256, 21845, (1 << 22) - 1] and list(i) == [0, 1, 65536, (1 << 24) - 1, 5]
    other = ev.copy()
    other[3] = ev[0]
    assert "event 3: got (rank 2, frame 0, index 0), expected (rank 2, frame 21845, index 16777215)" == HC.first_difference(other, ev)


# ---- merge and sink_layout against adder_amd.sharding on CPU tensors ---------------------------------------------------
class _FakeDist:
    """What exchange_stream_layout needs of torch.distributed, for ONE process that plays every rank in turn."""

    def __init__(self, all_offsets):
        import torch
        self.rows = [torch.from_numpy(np.ascontiguousarray(o)) for o in all_offsets]
        self.rank = 0

    def get_world_size(self, group=None):
        return len(self.rows)

    def get_rank(self, group=None):
        return self.rank

    def all_gather(self, out, t, group=None):
        import torch
        assert torch.equal(t, self.rows[self.rank])
        for o, row in zip(out, self.rows):
            o.copy_(row)


def _naive_merge(streams, offsets):
    out = []
    T = offsets.shape[1] - 1
    for f in range(T):
        for r, ev in enumerate(streams):
            a, b = offsets[r, f] - offsets[r, 0], offsets[r, f + 1] - offsets[r, 0]
            out.append(ev[a:b])
    return np.concatenate(out)


@pytest.mark.parametrize("T,empty_rank", HC.MERGE_SHAPES)
@pytest.mark.parametrize("starts", [(0, 0, 0), HC.MERGE_STARTS])
def test_merge_and_sink_layout_equal_sharding(T, empty_rank, starts, monkeypatch):
    import torch
    from adder_amd import sharding
    case = HC.merge_case(T, empty_rank, starts)
    streams, offsets = case["streams"], case["offsets"]
    got, moffs, dst = HO.merge(streams, offsets, HC.MERGE_BASE)
    assert np.array_equal(got, _naive_merge(streams, offsets))
    rebased = offsets - offsets[:, :1]
    want_ev, want_offs = sharding.merge_frame_major([(_i32(s), torch.from_numpy(o.copy())) for s, o in zip(streams, rebased)])
    assert torch.equal(_i32(got), want_ev)
    assert np.array_equal(moffs - HC.MERGE_BASE, want_offs.numpy())
    # the layout exchange, rank by rank, and the consumer side: every rank places its own segments
    fake = _FakeDist(rebased)
    monkeypatch.setattr(sharding, "dist", fake)
    placed = torch.full((len(got), 3), -1, dtype=torch.int32)
    for r in range(case["world"]):
        fake.rank = r
        frame_base, my_base = sharding.exchange_stream_layout(fake.rows[r])
        dest, merged, pos = HO.sink_layout(offsets, r, file_pos=HC.MERGE_BASE)
        assert np.array_equal(frame_base.numpy() + HC.MERGE_BASE, merged) and pos == merged[-1]
        assert np.array_equal(my_base.numpy() + HC.MERGE_BASE, dest)
        assert np.array_equal(my_base.numpy(), dst[r])
        sharding.place_segments(placed, _i32(streams[r]), fake.rows[r], my_base)
    assert torch.equal(placed, want_ev)


def test_an_altered_byte_or_entry_is_noticed():
    """What the comparisons above are worth: one byte of a record, one event of a merge."""
    ev = HC.wire_events(5, 3)
    good = HO.wire_bytes(ev, 11)
    for k in range(len(good)):
        bad = good.copy()
        bad[k] ^= 1
        assert bad.tobytes() != O.raw_events(ev, 3)
    case = HC.merge_case(9)
    got, _, _ = HO.merge(case["streams"], case["offsets"])
    want = _naive_merge(case["streams"], case["offsets"])
    for k in (0, len(got) // 2, len(got) - 1):
        bad = got.copy()
        bad[k]["t"] ^= 1
        assert not np.array_equal(bad, want) and HC.first_difference(bad, want).startswith(f"event {k}:")


# ---- the cases' properties --------------------------------------------------------------------------------------------
def _offsets_sound(offsets, starts):
    assert (np.diff(offsets, axis=1) >= 0).all() and list(offsets[:, 0]) == list(starts)


@pytest.mark.parametrize("T,empty_rank", HC.MERGE_SHAPES)
def test_merge_cases(T, empty_rank):
    assert [t for t, _ in HC.MERGE_SHAPES] == [1, HC.MERGE_TILE - 1, HC.MERGE_TILE, HC.MERGE_TILE + 1, 2 * HC.MERGE_TILE + 1]
    case = HC.merge_case(T, empty_rank, HC.MERGE_STARTS)
    counts, offsets = case["counts"], case["offsets"]
    _offsets_sound(offsets, HC.MERGE_STARTS)
    assert len(set(HC.MERGE_STARTS)) == 3 and min(HC.MERGE_STARTS) > 0 and max(HC.MERGE_STARTS) > 1 << 32
    assert set(np.unique(counts)) <= set(HC.MERGE_COUNTS)
    assert [len(s) for s in case["streams"]] == list(counts.sum(1)) == list(offsets[:, -1] - offsets[:, 0])
    if empty_rank is not None:
        assert counts[empty_rank].sum() == 0
    if T > 8:
        assert (counts.sum(0) == 0).any() and (counts == 0).sum() > T and (counts == 300).sum() > 10
    if T > HC.MERGE_TILE:   # the carry is not zero and the frames behind the first tile hold events that it moves
        assert counts[:, :HC.MERGE_TILE].sum() > 0 and counts[:, HC.MERGE_TILE:].sum() > 0
    # the three caps of the capacity arm
    if T == HC.MERGE_TILE + 1:
        case = HC.merge_case(T, None)
        merged, _, dst = HO.merge(case["streams"], case["offsets"])
        at, short, inside = HC.capacity_cuts(case)
        starts = set(dst[case["counts"] > 0].tolist())
        assert at in starts and short not in starts and inside not in starts and short == at - 1 and at < inside < len(merged) - 300


def test_pair_walk_case():
    case = HC.pair_walk_case()
    pairs = case["world"] * case["T"]
    assert case["world"] == 3 and HC.GRID_ROWS < pairs <= HC.GRID_ROWS + 3
    flat = case["counts"].reshape(-1)
    assert (flat[HC.GRID_ROWS:] > 0).all() and flat[0] > 0      # row 0 of the grid walks to a second, non-empty pair
    assert (flat == 0).mean() > 0.5 and 50_000 < flat.sum() < 150_000
    _offsets_sound(case["offsets"], (0, 0, 0))


@pytest.mark.parametrize("channels", [1, 3])
def test_sink_cases_reach_every_byte_phase(channels):
    rec = 9 if channels == 1 else 11
    chunks = HC.sink_case(channels)
    assert [c["nf"] for c in chunks] == [5, 70]
    sizes = set()
    for ch in chunks:
        _offsets_sound(ch["offsets"], HC.SINK_LEAD)
        sizes |= set(np.unique(ch["counts"]).tolist())
        for r, s in enumerate(ch["streams"]):
            assert len(s) == ch["offsets"][r, -1] and (HC.source_of(s[: HC.SINK_LEAD[r]])[0] == HC.FILLER_RANK).all()
    assert sizes == set(HC.SINK_SIZES) == {0, 1, 2, 3, HC.WIRE_EVENTS - 1, HC.WIRE_EVENTS, HC.WIRE_EVENTS + 1, 2 * HC.WIRE_EVENTS + 1}
    for header in HC.SINK_HEADERS:
        dests, merged, poss, body = HC.sink_expected(chunks, rec)
        heads, tails = HC.byte_phases(chunks, dests, rec, header)
        assert heads == {0, 1, 2, 3} and tails == {0, 1, 2, 3}, (header, heads, tails)
        assert merged[1][0] == poss[0] > 0 and poss[1] * rec == len(body)    # *d_file_pos carries over
        # the restatement's image: every rank scatters its own segments; together they are the merged stream's records
        image = np.full(header + len(body) + 16, 0xEE, np.uint8)
        for ch, d in zip(chunks, dests):
            for r in range(HC.SINK_WORLD):
                _, over = HO.scatter_image(image, ch["streams"][r], ch["offsets"][r], d[r], rec, header)
                assert not over
        assert (image[:header] == 0xEE).all() and (image[header + len(body):] == 0xEE).all()
        assert np.array_equal(image[header:header + len(body)], body)


def test_scatter_image_drops_cut_blocks_whole():
    chunks = HC.sink_case(1)
    dests, _, poss, body = HC.sink_expected(chunks, 9)
    ch, d = chunks[0], dests[0]
    full = np.full(len(body) + 64, 0xEE, np.uint8)
    for r in range(HC.SINK_WORLD):
        HO.scatter_image(full, ch["streams"][r], ch["offsets"][r], d[r], 9, 3)
    cap = 3 + (poss[0] // 2) * 9 + 4
    cut = np.full(len(body) + 64, 0xEE, np.uint8)
    dropped = False
    for r in range(HC.SINK_WORLD):
        _, over = HO.scatter_image(cut, ch["streams"][r], ch["offsets"][r], d[r], 9, 3, out_cap=cap, block=HC.WIRE_EVENTS)
        dropped |= over
    assert dropped and (cut[cap:] == 0xEE).all()
    same = cut == full
    assert same[:cap].any() and not same[:cap].all()      # some blocks below the cap are there, a cut one is not
    assert ((cut == 0xEE) | same).all()                   # what is there is right


def test_stride_case_needs_a_second_pass():
    case = HC.stride_case(256)
    assert case["n"] > case["grid"] * HC.WIRE_EVENTS and case["n"] == (case["grid"] + 1) * HC.WIRE_EVENTS + 1
    assert case["n"] * 12 < 14_000_000 and len(case["events"]) == case["n"]
    r, f, i = HC.source_of(case["events"][-3:])
    assert list(i) == [case["n"] - 3, case["n"] - 2, case["n"] - 1]


# ---- the row-chunk search ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", sorted(HC.CHUNK_CONTEXTS))
@pytest.mark.parametrize("kind", HC.CHUNK_EVENT_SETS)
def test_chunk_cases_and_chunk_offsets(ctx, kind):
    W, H, y0, y1, cr = HC.CHUNK_CONTEXTS[ctx]
    rows = y1 - y0
    nc = (rows + cr - 1) // cr
    assert y0 > 0 and y1 < H
    ev = HC.chunk_events(kind, y0, y1)
    y = ev["y"].astype(np.int64)
    assert (np.diff(y) >= 0).all() and (len(y) == 0 or (y0 <= y.min() and y.max() < y1))
    n = len(y)
    got = HO.chunk_offsets(ev["y"], y0, cr, nc, n)
    want = [sum(1 for v in y if v < y0 + c * cr) for c in range(nc)] + [n]
    assert list(got) == want and got.dtype == np.uint32
    if kind == "gaps":
        per_row = np.bincount(y - y0, minlength=rows)
        assert per_row[:7].sum() == 0 and per_row[-9:].sum() == 0 and per_row[rows // 2: rows // 2 + 11].sum() == 0
        assert per_row[7] + per_row[8] > 0
    assert {"none": n == 0, "one": n == 1, "one_row": n > 1 and len(set(y)) == 1}.get(kind, n > rows)


def test_chunk_contexts_cover_the_edges():
    shapes = {k: ((y1 - y0), cr) for k, (_, _, y0, y1, cr) in HC.CHUNK_CONTEXTS.items()}
    assert {cr for _, cr in shapes.values()} == {1, 5, 64}
    assert any(rows % cr for rows, cr in shapes.values())
    rows, cr = shapes["band300_rows1"]
    assert rows == 300 and cr == 1 and rows + 1 > HC.CHUNK_THREADS     # 301 entries: two workgroups


# ---- the frame ring past 255 row chunks ---------------------------------------------------------------------------------
def test_ring_clip_has_every_count_residue_and_chunk_offsets_equal_the_oracles():
    """The hand-over's copy ends in a tail of (3 n) & 3 dwords: the clip's frames must have event counts of every residue
    mod 4 (HC.RING_SEED was chosen for that).  The oracle's row chunks of the same frames check chunk_offsets."""
    assert HC.RING_H + 1 > HC.CHUNK_THREADS
    clip = HC.ring_clip()
    ov = HC.ring_oracle()
    residues = set()
    for f in clip:
        ev, chunks = ov.integrate_matrix(f, want_chunks=True)
        residues.add(len(ev) % 4)
        assert np.array_equal(chunks, HO.chunk_offsets(ev["y"], 0, 1, HC.RING_H, len(ev)))
    assert residues == {0, 1, 2, 3}
