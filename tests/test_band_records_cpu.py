"""The band records cases (tests/band_records_cases.py) reach the edges they are there for -- checked on the CPU, with
the oracle and numpy alone, so that a change of the generator that loses a case's point fails here and not silently on
the GPU."""
import numpy as np
import pytest

from oracle import oracle as O
import band_records_cases as BC

D_EMPTY = 0xFF


def _band_of(c, ev):
    """Index of the band every event lies in."""
    edges = np.array([b[1] for b in c["bands"]])
    return np.searchsorted(edges, ev["y"], side="right")


def test_constants_and_time_modes_are_the_products():
    from adder_amd import sharding
    assert (BC.DELTA_T, BC.ABSOLUTE_T) == (O.DELTA_T, O.ABSOLUTE_T) and BC.KW["multi_mode"] == O.COLLAPSE
    assert BC.WAVE_UNITS == 128 and BC.EXPAND_SEGS % 2 == 0 and BC.MAX_CHUNK <= 64
    for H, n in ((13, 3), (24, 4), (48, 3), (10, 2), (17, 17)):
        assert BC.row_bands(H, n) == sharding.row_bands(H, n)


@pytest.mark.parametrize("name", BC.NAMES)
def test_shapes_are_the_ones_the_table_names(name):
    c = BC.case(name)
    T, H, W, Cn = c["clip"].shape
    assert (W, H, Cn) == (c["W"], c["H"], c["Cn"]) and T == sum(c["chunks"]) and c["clip"].dtype == np.uint8
    assert max(c["chunks"]) <= BC.MAX_CHUNK
    bands = c["bands"]
    assert bands[0][0] == 0 and bands[-1][1] == H and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
    assert all(y1 > y0 for y0, y1 in bands)
    quantum = BC.EXPAND_SEGS * BC.WAVE_UNITS
    for (y0, y1), nseg in zip(bands, c["segments"]):
        units = (y1 - y0) * W * Cn
        assert nseg % BC.EXPAND_SEGS == 0 and (nseg - BC.EXPAND_SEGS) * BC.WAVE_UNITS < units <= nseg * BC.WAVE_UNITS
        assert nseg * BC.WAVE_UNITS == (units + quantum - 1) // quantum * quantum
    if name in BC.SEGMENTS:
        assert c["segments"] == BC.SEGMENTS[name]
    rowlen = W * Cn
    if name == "one_row_bands_16":
        assert len(bands) == BC.MAX_BANDS and all(y1 - y0 == 1 for y0, y1 in bands)
    if name == "one_row_bands_17":
        assert len(bands) == BC.MAX_BANDS + 1 and all(y1 - y0 == 1 for y0, y1 in bands)
    if name == "narrow_uneven":
        assert rowlen < 2 * BC.WAVE_UNITS and bands[1][1] - bands[1][0] == 1
        assert BC.MAX_CHUNK in c["chunks"] and 1 in c["chunks"] and c["chunks"].index(1) not in (0, len(c["chunks"]) - 1)
    if name == "wide_uneven":
        assert rowlen >= 2 * BC.WAVE_UNITS and {BC.MAX_CHUNK - 1, BC.MAX_CHUNK, 1} <= set(c["chunks"])
    if name == "rowlen_256":
        assert rowlen == 2 * BC.WAVE_UNITS
    if name == "rowlen_255":
        assert rowlen == 2 * BC.WAVE_UNITS - 1
    if name == "rgb":
        assert Cn == 3 and 1 in c["chunks"]
    if name == "segments_1024":  # one full trip of adder_log_bases_kernel (1024 segments per trip), no padding in it
        assert (bands[0][1] - bands[0][0]) * rowlen == 1024 * BC.WAVE_UNITS
    if name == "segments_1040":  # 1032 segments of units, padded to 1040: the second trip
        assert (bands[0][1] - bands[0][0]) * rowlen == 1032 * BC.WAVE_UNITS


@pytest.mark.parametrize("name", BC.NAMES)
def test_changed_units_per_segment_reach_the_census(name):
    """0, 1, 32, 33 and a whole segment (kWaveUnits, or every unit of a band shorter than that) in at least one band;
    a stretch of identical frames; clips of six frames and more have a cut."""
    c = BC.case(name)
    full = []
    for r, (y0, y1) in enumerate(c["bands"]):
        seen = set(np.unique(BC.changed_units(c, r)).tolist())
        whole = min(BC.WAVE_UNITS, (y1 - y0) * c["W"] * c["Cn"])
        if set(BC.CENSUS) | {whole} <= seen:
            full.append(r)
    assert full, "no band reaches 0, 1, 32, 33 and a whole segment"
    if max((y1 - y0) * c["W"] * c["Cn"] for y0, y1 in c["bands"]) >= BC.WAVE_UNITS:
        assert any(BC.WAVE_UNITS in np.unique(BC.changed_units(c, r)) for r in range(len(c["bands"])))
    T = c["clip"].shape[0]
    flat = c["clip"].reshape(T, -1)
    same = (flat[1:] == flat[:-1]).all(axis=1)
    assert same.any(), "no identical frames"
    if T >= 6:
        assert (flat[1:] != flat[:-1]).all(axis=1).any(), "no cut"
    assert (flat == 0).any(axis=1).all(), "a frame without black pixels"


@pytest.mark.parametrize("time_mode", BC.TIME_MODES, ids=BC.TIME_IDS.get)
@pytest.mark.parametrize("name", BC.NAMES)
def test_oracle_events_have_fillers_past_the_first_chunk(name, time_mode):
    """D_EMPTY fillers (their t is the frame's running_t: the frame table) in a chunk other than the first -- in a frame
    other than the first where the case has one chunk."""
    c = BC.case(name, time_mode)
    per = BC.oracle_events(name, time_mode)
    assert len(per) == sum(c["chunks"]) and sum(len(e) for e in per) > 0
    first = c["chunks"][0] if len(c["chunks"]) > 1 else 1
    later = np.concatenate(per[first:])
    assert (later["d"] == D_EMPTY).any()
    fillers = [(f, e[e["d"] == D_EMPTY]) for f, e in enumerate(per) if (e["d"] == D_EMPTY).any()]
    # ... and the fillers' t does depend on the frame: two frames' fillers differ in it
    assert len({int(e["t"][0]) for _, e in fillers}) == len(fillers)
    # every chunk has events (a one-frame chunk too)
    f0 = 0
    for nf in c["chunks"]:
        assert sum(len(e) for e in per[f0:f0 + nf]) > 0
        f0 += nf


@pytest.mark.parametrize("time_mode", BC.TIME_MODES, ids=BC.TIME_IDS.get)
def test_static_band_has_band_frames_without_events(time_mode):
    c = BC.case("static_band", time_mode)
    per = BC.oracle_events("static_band", time_mode)
    quiet_while_others_emit = 0
    for f, e in enumerate(per):
        counts = np.bincount(_band_of(c, e), minlength=len(c["bands"]))
        if counts[1] == 0 and counts.sum() > 0:
            quiet_while_others_emit += 1
            assert BC.STATIC_FRAMES[0] <= f < BC.STATIC_FRAMES[1]
    assert quiet_while_others_emit == BC.STATIC_FRAMES[1] - BC.STATIC_FRAMES[0]
    # the stretch crosses the chunk boundary: both chunks hold such frames
    assert BC.STATIC_FRAMES[0] < c["chunks"][0] < BC.STATIC_FRAMES[1]


@pytest.mark.parametrize("name", ["narrow_uneven", "rgb", "one_row_bands_17"])
def test_events_per_unit_follow_the_changed_units(name):
    """The generator's premise: in this regime a unit has events in exactly the frames in which its byte changes (the
    first frame: where it is not black) -- but for a unit that turns black right after a change, which the generator
    avoids -- so the changed units of a (segment, frame) are its records."""
    c = BC.case(name)
    per = BC.oracle_events(name, BC.DELTA_T)
    T, H, W, Cn = c["clip"].shape
    flat = c["clip"].reshape(T, -1)
    for f, e in enumerate(per):
        ch = np.where(e["c"] == 0xFF, 0, e["c"]).astype(np.int64)
        units = np.unique((e["y"].astype(np.int64) * W + e["x"]) * Cn + ch)
        want = np.flatnonzero(flat[f] != (flat[f - 1] if f else 0))
        assert np.array_equal(units, want), f


def test_records_constants_are_read_from_the_sources():
    """kernel_constants.records(): constants that stand on macros (the first #define of a name, the default behind its
    #ifndef) and the context's description slots; a missing name raises."""
    import kernel_constants
    k = kernel_constants.records()
    assert set(k) == set(kernel_constants.RECORDS_NAMES) | {"kBandDescSlots"} and all(v > 0 for v in k.values())
    assert (BC.WAVE_UNITS, BC.EXPAND_SEGS, BC.MAX_BANDS, BC.MAX_CHUNK, BC.DESC_SLOTS) == \
        (k["kWaveUnits"], k["kExpandSegs"], k["kMaxBands"], k["kMaxChunk"], k["kBandDescSlots"])
    text = ("#ifndef M_SEGS\n#define M_SEGS 16\n#endif\n#define M_SEGS 99  // (never the second)\n"
            "constexpr uint32_t kA = M_SEGS;\nconstexpr uint32_t kB = 64 * kA;\n")
    assert kernel_constants.parse_u32_constants(text, ("kA", "kB"), macros=True) == {"kA": 16, "kB": 1024}
    with pytest.raises(KeyError):
        kernel_constants.parse_u32_constants(text, ("kA",))
    with pytest.raises(KeyError):
        kernel_constants.parse_u32_constants(text, ("kA", "kMissing"), macros=True)
