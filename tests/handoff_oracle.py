"""A restatement in plain numpy of what the stream hand-off kernels compute (adder_kernels.hip: adder_wire_kernel,
adder_sink_layout_kernel + adder_wire_scatter_kernel, adder_merge_layout_kernel + adder_merge_copy_kernel,
adder_chunk_offsets_kernel), for the edge tests to compare with bit for bit.  Nothing of the library is imported here:
test_handoff_cpu.py checks this file against the independent implementations the project has (the oracle's and the host
library's raw sink, adder_amd.sharding on CPU tensors).  Everything is vectorised with cumsum / repeat: one case has
65 000 frames."""
import numpy as np

# AdderEvent (include/adder_hip.h), 12 bytes
EVENT_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("c", "u1"), ("d", "u1"), ("pad", "<u2"), ("t", "<u4")])
assert EVENT_DTYPE.itemsize == 12


def wire_bytes(events, rec):
    """The raw sink's records of `events` back to back (raw/stream.rs:101-120, bincode fixint big-endian) as a uint8 array:
    rec = 9: {x be16, y be16, d, t be32}; rec = 11: {x be16, y be16, 0x01, c, d, t be32}."""
    assert rec in (9, 11)
    n = len(events)
    out = np.zeros((n, rec), np.uint8)
    x, y, t = events["x"].astype(np.uint32), events["y"].astype(np.uint32), events["t"].astype(np.uint32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = x >> 8, x & 255, y >> 8, y & 255
    k = 4
    if rec == 11:
        out[:, 4], out[:, 5] = 1, events["c"]
        k = 6
    out[:, k] = events["d"]
    for j in range(4):
        out[:, k + 1 + j] = (t >> (24 - 8 * j)) & 255
    return out.reshape(-1)


def _layout(counts):
    """counts [R, T] -> (base [T + 1]: exclusive prefix of the frames' totals, before [R, T]: events of the lower ranks
    in the same frame)."""
    counts = np.asarray(counts, np.int64)
    base = np.zeros(counts.shape[1] + 1, np.int64)
    base[1:] = np.cumsum(counts.sum(0))
    return base, np.cumsum(counts, 0) - counts


def _segment_index(offsets_row):
    """For one rank's frame offsets [T + 1]: (frame of every event, its index inside the frame's segment)."""
    offsets_row = np.asarray(offsets_row, np.int64)
    counts = np.diff(offsets_row)
    frame_id = np.repeat(np.arange(len(counts)), counts)
    local = np.arange(int(counts.sum())) - (offsets_row[:-1] - offsets_row[0])[frame_id]
    return frame_id, local


def merge(streams, offsets, merged_base=0):
    """streams[r]: rank r's events of the chunk, beginning at ITS first event; offsets [R, T + 1]: the ranks' frame offsets
    (a row may start at any value).  -> (merged events: frame-major, rank order inside a frame; merged offsets [T + 1],
    continuing from merged_base; dst [R, T]: where rank r's segment of frame f starts in the merged chunk)."""
    offsets = np.asarray(offsets, np.int64)
    counts = np.diff(offsets, axis=1)
    assert (counts >= 0).all()
    base, before = _layout(counts)
    dst = base[:-1][None, :] + before
    out = np.zeros(int(base[-1]), EVENT_DTYPE)
    for r, ev in enumerate(streams):
        frame_id, local = _segment_index(offsets[r])
        assert len(ev) >= len(frame_id)
        out[dst[r][frame_id] + local] = ev[: len(frame_id)]
    return out, base + int(merged_base), dst


def sink_layout(all_offsets, rank, file_pos):
    """The sink per rank: all_offsets [R, nf + 1] of one chunk, file_pos = events the image holds before it.
    -> (dest [nf]: event index in the image of `rank`'s segment of every frame, merged offsets [nf + 1], new file_pos)."""
    counts = np.diff(np.asarray(all_offsets, np.int64), axis=1)
    base, before = _layout(counts)
    merged = base + int(file_pos)
    return merged[:-1] + before[rank], merged, int(merged[-1])


def scatter_image(image, events, offsets, dest, rec, header_bytes, out_cap=None, block=None):
    """Stores one rank's events of a chunk (events indexed by the VALUES of offsets [nf + 1]) as wire records at
    image[header_bytes + dest[f] * rec ...], in place.  out_cap / block: the kernel's capacity arm -- a block of `block`
    events of a frame's segment that would end beyond out_cap bytes is dropped WHOLE.  -> (image, a block was dropped)."""
    offsets = np.asarray(offsets, np.int64)
    frame_id, local = _segment_index(offsets)
    src = offsets[0] + np.arange(len(frame_id))
    where = np.asarray(dest, np.int64)[frame_id] + local   # event index in the image
    keep = np.ones(len(frame_id), bool)
    if out_cap is not None:
        counts = np.diff(offsets)
        blk0 = local - local % block                       # first event of the event's block, inside its segment
        blk_cnt = np.minimum(block, counts[frame_id] - blk0)
        keep = header_bytes + (where - local + blk0 + blk_cnt) * rec <= out_cap
    rows = wire_bytes(events[src[keep]], rec).reshape(-1, rec)
    pos = (header_bytes + where[keep] * rec)[:, None] + np.arange(rec)[None, :]
    image[pos] = rows
    return image, bool((~keep).any())


def chunk_offsets(y, row_begin, chunk_rows, num_chunks, n):
    """offsets[c] = first of the n y-sorted events with y >= row_begin + c * chunk_rows; offsets[num_chunks] = n."""
    y0 = row_begin + np.arange(num_chunks, dtype=np.int64) * chunk_rows
    out = np.empty(num_chunks + 1, np.uint32)
    out[:num_chunks] = np.searchsorted(np.asarray(y[:n], np.int64), y0, "left")
    out[num_chunks] = n
    return out
