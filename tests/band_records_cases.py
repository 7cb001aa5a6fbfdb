"""Seeded clips and band splits for the band records hand-off (adder_hip_integrate_records_device ->
adder_hip_expand_records_device / _wire_device; csrc/adder_kernels.hip: adder_slot_pack_kernel, adder_log_bases_kernel,
adder_log_pack_kernel, adder_band_layout_kernel, adder_expand_bands_kernel).  No GPU here: tests/test_band_records_cpu.py
checks on the CPU that every case reaches the edge it is there for, tests/test_gpu_band_records.py runs them.

A case is dict(name, W, H, Cn, time_mode, bands=[(y0, y1), ...], chunks=[nf, ...], clip, segments=[per band], why); the
clip is uint8 [sum(chunks)][H][W][Cn].  The regime is the lean one the records path requires: Collapse, ref_time =
delta_t_max = 255, c_thresh 0, crf 0 (KW / CRF below), so time_spanned == ref_time >= 255 and AbsoluteT takes the
lean-runs kernel like DeltaT does.

The clips are built per 128-unit SEGMENT of a band (a band's units in raster order, channels interleaved -- the frame
kernel's segments), not from synth_clip: in that regime a unit parks one record in exactly the frames in which its byte
changes, so the records of a (segment, frame) are the units changed there, and the expansion's two paths -- a PAIR of
segments together up to 32 records each, one segment at a time above -- are chosen by those counts.  A frame of a clip
is one of
  base   the first frame: random bytes, an eighth of them black;
  mixed  the segments of every band change 1, 32, 33, some other number, 0 and all of their units in turn (shifted by
         one from band to band and from frame to frame; shuffled in bands of twelve segments and more); a changed unit
         that was quiet the frame before turns black one time in four (so roots of intensity 0 start and end, and
         D_EMPTY fillers -- the flush of a root that had been popped -- take their t from the frame table), any other
         byte otherwise;
  still  the frame before it again, from frame 1 (a stretch of them where the clip is long enough);
  cut    every unit changes (clips of six frames and more).
`static_band` keeps its middle band still over frames 4 .. 13 (across the chunk boundary) while the outer bands go on.

Census of narrow_uneven on an MI355X (test_gpu_band_records.py::test_records_per_segment_reach_both_expansion_paths,
d_counts copied back, records in the high half; the same in both record kinds): in the chunks after the first (frames
37 .. 103) the records of every (segment, frame) of every band equal the units changed there; over the clip, rows 0 .. 13
(10.2 segments) and rows 14 .. 37 (18 segments) see 0, 1, 32, 33, 128 and about a hundred other counts between 2 and
127, the one-row band 13 .. 14 (100 units, one segment) 0, 1, 2, 7, 13, 15, 32, 33, 35 .. 83 and 100.  So (segment,
frame) pairs without a record, with 1 .. 32 records (expanded as a pair of segments) and with more (one segment at a
time) are all there, on either side of 32 exactly.  No case has a band whose whole CHUNK holds no record: static_band's
middle band is still over frames 4 .. 13, inside the chunks 0 .. 8 and 9 .. 17, which both have moving frames too.
test_wire_image_of_several_bands therefore cuts static_band into chunks of 4, 5, 4 and 5 frames: the middle band's
second and third chunk (frames 4 .. 8 and 9 .. 12) then park nothing, and their images end at the sixth section.
"""
import functools

import numpy as np

import kernel_constants

K = kernel_constants.records()
WAVE_UNITS, EXPAND_SEGS, MAX_BANDS, MAX_CHUNK = K["kWaveUnits"], K["kExpandSegs"], K["kMaxBands"], K["kMaxChunk"]
DESC_SLOTS = K["kBandDescSlots"]

DELTA_T, ABSOLUTE_T = 0, 1  # ADDER_TIME_* (include/adder_hip.h) == oracle.DELTA_T / ABSOLUTE_T
TIME_MODES = (DELTA_T, ABSOLUTE_T)
TIME_IDS = {DELTA_T: "delta_t", ABSOLUTE_T: "absolute_t"}
# HipVideo's arguments besides the plane, the band and the time mode (test_gpu_records.py's kw); multi_mode 1 = Collapse (ADDER_MULTI_COLLAPSE)
KW = dict(multi_mode=1, ref_time=255, delta_t_max=255, c_thresh_start=0, c_counter_start=0)
CRF = (0, 10)  # set_crf_parameters: c_thresh_max 0 (crf 0), the default velocity

CENSUS = (0, 1, 32, 33)  # ... and every unit of the segment: kWaveUnits where the band has a whole segment


def row_bands(height, world):
    """adder_amd.sharding.row_bands with chunk_rows 1 (that module needs torch; test_band_records_cpu compares them)."""
    base, extra = divmod(height, world)
    out, y = [], 0
    for r in range(world):
        y1 = y + base + (1 if r < extra else 0)
        out.append((y, y1))
        y = y1
    return out


def band_segments(W, Cn, band):
    """adder_hip_band_segments of a band: its units padded to whole groups of kExpandSegs segments."""
    quantum = EXPAND_SEGS * WAVE_UNITS
    units = (band[1] - band[0]) * W * Cn
    return (units + quantum - 1) // quantum * EXPAND_SEGS


# name -> (W, H, Cn, bands, chunks, seed, what the case is there for)
_TABLE = {
    "one_row_bands_16": (48, MAX_BANDS, 1, row_bands(MAX_BANDS, MAX_BANDS), [5, 2], 11,
                         "exactly kMaxBands bands: the single launch at its limit"),
    "one_row_bands_17": (48, MAX_BANDS + 1, 1, row_bands(MAX_BANDS + 1, MAX_BANDS + 1), [5, 2], 12,
                         "kMaxBands + 1 bands: one expansion launch per band"),
    "narrow_uneven": (100, 37, 1, [(0, 13), (13, 14), (14, 37)], [37, MAX_CHUNK, 1, 2], 13,
                      "rowlen < 2 kWaveUnits (several row ends per segment pair); a one-row band between large ones; "
                      "nf = kMaxChunk; a one-frame chunk"),
    "wide_uneven": (300, 13, 1, row_bands(13, 3), [MAX_CHUNK - 1, MAX_CHUNK, 1], 14,
                    "rowlen >= 2 kWaveUnits (one_wrap); nf 63 and 64: adder_slot_pack_kernel sums the frames before f, one "
                    "lane each"),
    "rowlen_256": (2 * WAVE_UNITS, 10, 1, row_bands(10, 2), [3], 15, "rowlen == 2 kWaveUnits: one_wrap just holds"),
    "rowlen_255": (2 * WAVE_UNITS - 1, 10, 1, row_bands(10, 2), [3], 16, "rowlen == 2 kWaveUnits - 1: one_wrap just fails"),
    "rgb": (50, 24, 3, row_bands(24, 4), [7, 1], 17, "11-byte wire records, channel numbering across bands"),
    "segments_1024": (512, 258, 1, [(0, 256), (256, 258)], [3, 1], 18,
                      "a band of exactly 1024 segments: one full trip of adder_log_bases_kernel"),
    "segments_1040": (512, 260, 1, [(0, 258), (258, 260)], [3, 1], 19,
                      "1032 segments padded to 1040: adder_log_bases_kernel's second trip and its carry"),
    "static_band": (64, 48, 1, row_bands(48, 3), [9, 9], 20, "(band, frame) pairs with no event and no record"),
}
NAMES = tuple(_TABLE)
# the segment counts the cases are there for: [per band]
SEGMENTS = {
    "one_row_bands_16": [16] * 16,
    "one_row_bands_17": [16] * 17,
    "segments_1024": [1024, 16],
    "segments_1040": [1040, 16],
}
STATIC_FRAMES = (4, 14)  # static_band: its middle band repeats frame 3 over these frames


def frame_kinds(T):
    kinds = ["base"] + ["mixed"] * (T - 1)
    if T >= 3:
        for f in range(1, 1 + max(1, T // 8)):
            kinds[f] = "still"
    if T >= 6:
        kinds[T - 3] = "cut"
    return kinds


def _other_byte(rng, old, black):
    """A byte != old for every entry: 0 where `black` (and old != 0), any other value otherwise."""
    new = (old.astype(np.int64) + rng.integers(1, 256, old.shape)) % 256  # != old
    nonzero = np.where(new == 0, (old.astype(np.int64) + 1) % 256, new)   # != old, and != 0 unless old == 255 ...
    nonzero = np.where(nonzero == 0, 1, nonzero)                          # ... then 1
    return np.where(black & (old != 0), 0, nonzero).astype(np.uint8)


_CYCLE = (1, 32, 33, -1, 0, WAVE_UNITS)  # -1: any count between 2 and the segment's size


def _mixed_band(rng, cur, may_black, phase):
    """cur: the band's units (flat uint8) of the frame before; returns the next frame's, changed per segment: segment s
    changes _CYCLE[s + phase] units (so a band of one segment reaches every count over its frames, and a pair of
    segments every neighbouring two), in random order where the band has two cycles' worth of segments."""
    out = cur.copy()
    nseg = (len(cur) + WAVE_UNITS - 1) // WAVE_UNITS
    counts = [_CYCLE[(s + phase) % len(_CYCLE)] for s in range(nseg)]
    if nseg >= 2 * len(_CYCLE):
        rng.shuffle(counts)
    for s, n in enumerate(counts):
        s0 = s * WAVE_UNITS
        size = min(WAVE_UNITS, len(cur) - s0)
        n = min(n, size) if n >= 0 else (int(rng.integers(2, size)) if size > 2 else size)
        if n == 0:
            continue
        idx = s0 + (np.arange(size) if n == size else np.sort(rng.choice(size, n, replace=False)))
        out[idx] = _other_byte(rng, cur[idx], may_black[idx] & (rng.integers(0, 4, n) == 0))
    return out


def make_clip(name):
    W, H, Cn, bands, chunks, seed, _ = _TABLE[name]
    rng = np.random.default_rng(seed)
    T = sum(chunks)
    clip = np.zeros((T, H, W, Cn), np.uint8)
    flat = clip.reshape(T, H, W * Cn)
    kinds = frame_kinds(T)
    mixed = 0
    for f, kind in enumerate(kinds):
        if kind == "base":
            v = rng.integers(1, 256, (H, W * Cn))
            flat[f] = np.where(rng.integers(0, 8, v.shape) == 0, 0, v)
            continue
        for r, (y0, y1) in enumerate(bands):
            cur = flat[f - 1, y0:y1].reshape(-1)
            # (a unit that turns black in the frame after it changed has no event there -- its new root was popped at
            # once and has not accumulated -- and parks no record: black only after a quiet frame, so that the units
            # changed are the records)
            may_black = (cur == flat[f - 2, y0:y1].reshape(-1)) if f >= 2 else np.zeros(cur.shape, bool)
            if kind == "still" or (name == "static_band" and r == 1 and STATIC_FRAMES[0] <= f < STATIC_FRAMES[1]):
                new = cur
            elif kind == "cut":
                new = _other_byte(rng, cur, may_black & (rng.integers(0, 4, cur.shape) == 0))
            else:
                new = _mixed_band(rng, cur, may_black, mixed + r)
            flat[f, y0:y1] = new.reshape(y1 - y0, W * Cn)
        mixed += kind == "mixed"
    return clip


@functools.lru_cache(maxsize=None)
def _shape_and_clip(name):
    W, H, Cn, bands, chunks, _, why = _TABLE[name]
    clip = make_clip(name)
    clip.setflags(write=False)
    return dict(name=name, W=W, H=H, Cn=Cn, bands=list(bands), chunks=list(chunks), clip=clip, why=why,
                segments=[band_segments(W, Cn, b) for b in bands])


def case(name, time_mode=DELTA_T):
    """The case dict; the clip (read-only, shared) and the split do not depend on the time mode."""
    return dict(_shape_and_clip(name), time_mode=time_mode)


def all_cases():
    return [case(n, tm) for n in NAMES for tm in TIME_MODES]


def changed_units(c, r):
    """[T - 1][segments of band r] units of the segment whose byte differs from the frame before (frames 1 .. T - 1)."""
    y0, y1 = c["bands"][r]
    T = c["clip"].shape[0]
    u = c["clip"][:, y0:y1].reshape(T, -1)
    diff = u[1:] != u[:-1]
    nseg = (diff.shape[1] + WAVE_UNITS - 1) // WAVE_UNITS
    pad = np.zeros((T - 1, nseg * WAVE_UNITS), bool)
    pad[:, :diff.shape[1]] = diff
    return pad.reshape(T - 1, nseg, WAVE_UNITS).sum(axis=2)


@functools.lru_cache(maxsize=None)
def oracle_events(name, time_mode):
    """The oracle's events of the whole plane, one array per frame (computed once per case and time mode; shared)."""
    from oracle import oracle as O
    c = _shape_and_clip(name)
    ov = O.Video(c["W"], c["H"], c["Cn"], time_mode=time_mode, multi_mode=O.COLLAPSE, ref_time=KW["ref_time"],
                 delta_t_max=KW["delta_t_max"])
    ov.ensure_capacity(8)
    ov.set_crf_parameters(*CRF)
    ov.reset_c_thresh(0)
    out = [ov.integrate_matrix(f) for f in c["clip"]]
    for e in out:
        e.setflags(write=False)
    return out
