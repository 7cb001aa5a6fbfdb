"""Synthetic, seeded inputs for edge tests of the stream hand-off kernels: plain device buffers that drive the entry points
without a transcoder in the loop (test_handoff_cpu.py checks the builders).  Shapes come from the kernels' named constants
(kernel_constants.handoff()), so they move with a retune.

Every event is recognisable: its source position (rank, frame, index inside the rank's segment of the frame) is packed
into t and x, so a misplaced event names where it came from (source_of)."""
import numpy as np

import handoff_oracle as HO
import kernel_constants

K = kernel_constants.handoff()
WIRE_EVENTS = K["kWireEvents"]          # events per workgroup pass of the serialisers
MERGE_TILE = K["kMergeTileFrames"]      # frames per tile of the merge layout's prefix
GRID_ROWS = K["kMaxGridRows"]           # gridDim.y at most
CHUNK_THREADS = K["kBlockThreads"]      # row chunks one workgroup of the chunk search takes
SCATTER_GROUPS_PER_CU = K["kScatterGroupsPerCu"]

FILLER_RANK = 3  # events that no kernel may ever move (in front of a rank's first event)


def make_events(rank, frame, index, channels=1, y=None):
    """Events marked (rank < 4, frame < 2^22, index < 2^24): t = (frame & 255) << 24 | index,
    x = rank << 14 | frame >> 8.  c = index % channels (0xff, "no channel", on one channel), d and pad vary with index."""
    frame, index = np.asarray(frame, np.int64), np.asarray(index, np.int64)
    assert rank < 4 and (frame < (1 << 22)).all() and (index < (1 << 24)).all()
    ev = np.zeros(len(index), HO.EVENT_DTYPE)
    ev["t"] = ((frame & 255) << 24) | index
    ev["x"] = (rank << 14) | (frame >> 8)
    ev["y"] = (index * 7 + frame) & 0xffff if y is None else y
    ev["c"] = 0xff if channels == 1 else index % channels
    ev["d"] = (index * 13 + rank) & 0xff
    ev["pad"] = (index * 31 + 7) & 0xffff
    return ev


def source_of(ev):
    """(rank, frame, index) of marked events."""
    t, x = ev["t"].astype(np.int64), ev["x"].astype(np.int64)
    return x >> 14, ((x & 0x3fff) << 8) | (t >> 24), t & 0xffffff


def describe(ev):
    r, f, i = source_of(ev[:1])
    return f"(rank {int(r[0])}, frame {int(f[0])}, index {int(i[0])})"


def first_difference(got, want):
    """A message naming the first event of `got` that differs from `want` (equal lengths)."""
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1, 3) != want.view(np.uint32).reshape(-1, 3))
    if len(bad) == 0:
        return "equal"
    k = int(bad[0]) // 3
    return f"event {k}: got {describe(got[k:k + 1])}, expected {describe(want[k:k + 1])}"


def streams_from_counts(counts, starts, channels=1, lead=None):
    """counts [R, T] -> (streams: rank r's marked events, frame-major, preceded by lead[r] filler events; offsets [R, T + 1]
    starting at starts[r])."""
    counts = np.asarray(counts, np.int64)
    R, T = counts.shape
    offsets = np.zeros((R, T + 1), np.int64)
    offsets[:, 1:] = np.cumsum(counts, 1)
    streams = []
    for r in range(R):
        frame_id = np.repeat(np.arange(T), counts[r])
        local = np.arange(len(frame_id)) - offsets[r, :-1][frame_id]
        ev = make_events(r, frame_id, local, channels)
        if lead is not None and lead[r]:
            ev = np.concatenate([make_events(FILLER_RANK, np.zeros(lead[r], np.int64), np.arange(lead[r]), channels), ev])
        streams.append(ev)
    return streams, offsets + np.asarray(starts, np.int64)[:, None]


# ---- the multi-GPU merge ------------------------------------------------------------------------------------------
MERGE_WORLD = 3
MERGE_COUNTS = (0, 0, 1, 2, 5, 300)
# (T, a rank without any event): one frame, the 256-frame tile minus / exactly / plus one, two tiles and a frame
MERGE_SHAPES = ((1, None), (MERGE_TILE - 1, 0), (MERGE_TILE, None), (MERGE_TILE + 1, 1), (2 * MERGE_TILE + 1, 2))
MERGE_STARTS = (7, 1_000_003, (1 << 33) + 5)   # a chunk of a longer stream: every rank's offsets start elsewhere
MERGE_BASE = 12_345


def merge_case(T, empty_rank=None, starts=(0, 0, 0), seed=0):
    """world = 3, per-(rank, frame) counts drawn from MERGE_COUNTS; every 7th frame (f % 7 == 3) is empty on every rank."""
    rng = np.random.default_rng([seed, T])
    counts = rng.choice(np.array(MERGE_COUNTS, np.int64), (MERGE_WORLD, T))
    counts[:, 3::7] = 0
    if empty_rank is not None:
        counts[empty_rank] = 0
    streams, offsets = streams_from_counts(counts, starts)
    return dict(world=MERGE_WORLD, T=T, counts=counts, streams=streams, offsets=offsets)


def pair_walk_case(seed=1):
    """world * T just above the grid's row limit: the copy kernel's blockIdx.y walks to a second pair.  Counts are mostly
    0; the pairs beyond the limit and the pair that shares a row with the first of them hold events."""
    world = MERGE_WORLD
    T = GRID_ROWS // world + 1
    rng = np.random.default_rng(seed)
    counts = rng.choice(np.array((0, 0, 0, 0, 0, 0, 1, 2, 5, 7), np.int64), (world, T))
    flat = counts.reshape(-1)
    flat[0] = 2
    flat[GRID_ROWS:] = np.arange(3, 3 + len(flat) - GRID_ROWS)
    streams, offsets = streams_from_counts(counts, (0,) * world)
    return dict(world=world, T=T, counts=counts, streams=streams, offsets=offsets)


def capacity_cuts(case):
    """For the merge's capacity arm: (cap at a segment's boundary, one event short of it, inside the segment), at a
    300-event segment in the middle of the merged stream whose predecessor in the stream holds several events."""
    _, _, dst = HO.merge(case["streams"], case["offsets"])
    counts = case["counts"]
    T = case["T"]
    for f in range(T // 2, T):
        for r in range(1, case["world"]):
            if counts[r, f] == max(MERGE_COUNTS) and counts[r - 1, f] > 1:
                b = int(dst[r, f])
                return b, b - 1, b + int(counts[r, f]) // 2
    raise AssertionError("no such segment")


# ---- the sink per rank: layout + wire scatter ----------------------------------------------------------------------
SINK_WORLD = 3
SINK_SIZES = (0, 1, 2, 3, WIRE_EVENTS - 1, WIRE_EVENTS, WIRE_EVENTS + 1, 2 * WIRE_EVENTS + 1)
SINK_CHUNKS = (5, 70)
SINK_HEADERS = (0, 1, 2, 3, 33)
SINK_LEAD = (0, 3, 5)   # rank r's event buffer begins with this many filler events: its offsets start there


def sink_case(channels, seed=2):
    """Two successive chunks (nf = 5, 70) of three ranks; segment sizes drawn from SINK_SIZES.  -> a list of chunks,
    each dict(nf, streams, offsets [3, nf + 1])."""
    chunks = []
    for k, nf in enumerate(SINK_CHUNKS):
        rng = np.random.default_rng([seed, channels, k])
        counts = rng.choice(np.array(SINK_SIZES, np.int64), (SINK_WORLD, nf))
        streams, offsets = streams_from_counts(counts, SINK_LEAD, channels, lead=SINK_LEAD)
        chunks.append(dict(nf=nf, counts=counts, streams=streams, offsets=offsets))
    return chunks


def sink_expected(chunks, rec):
    """The restatement over the chunks: (per chunk and rank dest, per chunk merged offsets, per chunk file_pos after it,
    the merged stream's wire bytes)."""
    file_pos, dests, merged, poss, body = 0, [], [], [], []
    for ch in chunks:
        d = []
        for r in range(SINK_WORLD):
            dest, mo, new_pos = HO.sink_layout(ch["offsets"], r, file_pos)
            d.append(dest)
        dests.append(d)
        merged.append(mo)
        ev, _, _ = HO.merge([s[lead:] for s, lead in zip(ch["streams"], SINK_LEAD)], ch["offsets"])
        body.append(HO.wire_bytes(ev, rec))
        file_pos = new_pos
        poss.append(file_pos)
    return dests, merged, poss, np.concatenate(body)


def byte_phases(chunks, dests, rec, header_bytes):
    """{(first byte of a non-empty segment in the image) & 3} and {(bytes after the head) & 3} over all segments."""
    heads, tails = set(), set()
    for ch, d in zip(chunks, dests):
        for r in range(SINK_WORLD):
            n = ch["counts"][r]
            a0 = header_bytes + d[r] * rec
            for a, c in zip(a0[n > 0], n[n > 0]):
                for e0 in range(0, int(c), WIRE_EVENTS):
                    b = min(WIRE_EVENTS, int(c) - e0) * rec
                    p = int(a + e0 * rec) & 3
                    head = min((4 - p) & 3, b)
                    heads.add(p)
                    tails.add((b - head) & 3)
    return heads, tails


def stride_case(cus):
    """One frame, one rank: more events than the scatter's fixed grid (4 workgroups per CU) takes in one pass of
    1024-event blocks, plus a block and one event."""
    n = SCATTER_GROUPS_PER_CU * cus * WIRE_EVENTS + WIRE_EVENTS + 1
    ev = make_events(0, np.zeros(n, np.int64), np.arange(n))
    return dict(n=n, events=ev, offsets=np.array([[0, n]], np.int64), grid=SCATTER_GROUPS_PER_CU * cus)


# ---- the wire kernel -----------------------------------------------------------------------------------------------
WIRE_COUNTS = (1, 3, WIRE_EVENTS, WIRE_EVENTS + 1)


def wire_events(n, channels, seed=3):
    rng = np.random.default_rng([seed, n, channels])
    ev = make_events(1, rng.integers(0, 1 << 22, n), np.arange(n), channels)
    ev["y"] = rng.integers(0, 0xffff, n)
    return ev


def extreme_events(channels):
    """Field values at their ends: x = y = 0xfffe, t = 0xffffffff, d = 255, and zeros; c = 0 on three channels."""
    ev = np.zeros(4, HO.EVENT_DTYPE)
    ev["x"], ev["y"] = [0xfffe, 0, 0xfffe, 0x0102], [0xfffe, 0xfffe, 0, 0x0304]
    ev["t"], ev["d"] = [0xffffffff, 0, 0x80000001, 0x0a0b0c0d], [255, 0, 128, 5]
    ev["c"] = 0xff if channels == 1 else [0, 2, 1, 0]
    ev["pad"] = 0xbeef
    return ev


# ---- the row-chunk search ------------------------------------------------------------------------------------------
# (W, H, row_begin, row_end, chunk_rows): a row band, a chunk height that does not divide it, and more than 255 chunks
CHUNK_CONTEXTS = {
    "band67_rows5": (8, 100, 10, 77, 5),
    "band67_rows64": (8, 100, 10, 77, 64),
    "band67_rows1": (8, 100, 10, 77, 1),
    "band300_rows1": (8, 400, 37, 337, 1),
}
CHUNK_EVENT_SETS = ("none", "one", "one_row", "gaps", "dense")


def chunk_events(kind, row_begin, row_end, seed=4):
    """y-sorted events of a band.  gaps: no events in the top rows, in a run of rows in the middle and in the bottom rows."""
    rows = row_end - row_begin
    rng = np.random.default_rng([seed, rows])
    if kind == "none":
        y = np.zeros(0, np.int64)
    elif kind == "one":
        y = np.array([row_begin + rows // 2])
    elif kind == "one_row":
        y = np.full(40, row_begin + rows // 3)
    elif kind == "gaps":
        live = np.arange(row_begin + 7, row_end - 9)
        live = live[(live < row_begin + rows // 2) | (live >= row_begin + rows // 2 + 11)]
        y = np.sort(rng.choice(live, 3 * rows))
    else:
        y = np.sort(rng.integers(row_begin, row_end, 5 * rows))
    return make_events(0, np.zeros(len(y), np.int64), np.arange(len(y)), y=y)


# ---- the frame ring past 255 row chunks ----------------------------------------------------------------------------
RING_W, RING_H, RING_FRAMES = 8, 300, 12
RING_SEED = 0  # chosen on the CPU with the oracle alone (test_handoff_cpu.py asserts the property it was chosen for)


# the context of both sides: lean kernels, lossy (the existing ring tests' configuration)
RING_MODES = dict(time_mode=1, multi_mode=1, ref_time=255, delta_t_max=255, chunk_rows=1)  # AbsoluteT, Collapse
RING_CRF = (7, 7, 2)  # c_thresh_max, c_increase_velocity, c_thresh baseline


def ring_clip():
    import clips
    return clips.make_clip("runs", RING_FRAMES, RING_H, RING_W, 1, seed=RING_SEED)


def ring_oracle():
    from oracle import oracle as O
    assert (O.ABSOLUTE_T, O.COLLAPSE) == (RING_MODES["time_mode"], RING_MODES["multi_mode"])
    ov = O.Video(RING_W, RING_H, 1, **RING_MODES)
    ov.ensure_capacity(34)
    ov.set_crf_parameters(*RING_CRF[:2])
    ov.reset_c_thresh(RING_CRF[2])
    return ov
