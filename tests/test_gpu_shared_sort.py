"""The stable pair sort (hipcub::DeviceRadixSort::SortPairs over uint32 keys and indices) and the offset scan behind it,
which every event tool runs in the same form, at the sort's size edges, through the public binding of each tool that
has no size-edge test of it: DVS convert and dvs_sort, the latest-event player, the adder-viz player, stream migration
(Forward and Inverse), adder-info in AbsoluteT and the framer's feature pass.  Every result is compared bit for bit
with the tool's restatement in tests/.  The tests hold whether each tool writes the sort out itself, as now, or all
call one copy (profiles/shared_sort_refactor.md).

Planes 2x4, 32x16 and 346x260 of one channel give 4, 10 and 17 key bits (test_gpu_source_chain.PLANES).  Record counts
1, 1024, 1025 and 2600: one record, rocPRIM's last single-block size (sparse_cases.BLOCK_SORT_ITEMS = 256 * 4), its
first merge size, and several blocks with a part.  Three planes at 2600 records and four counts at 32x16, per tool.
Half the records of a stream go to three hot pixels (the first, the middle and the last unit), the rest walk the plane
in a shuffled order, so runs of equal keys cross the 256-record block edges; one seed per case.

The onesweep path (past sparse_cases.MERGE_SORT_LIMIT = 1 Mi records) is not run here: the restatements are Python
loops and take minutes at that size.  tests/test_gpu_sparse_edges.py and the 1080p cases of tests/test_gpu_dvs.py
keep covering it."""
import numpy as np
import pytest

import adder_stream_np as S
import dvs_oracle as DR
import framer_features_cases as FK
import framer_features_oracle as FR
import stream_tools_oracle as SR
import viz_player_cases as VK
from sparse_cases import BLOCK_SORT_ITEMS, sort_path
from test_gpu_dvs import as_list
from test_gpu_framer_features import Dev
from test_gpu_player import bits, make_player, meta_of, random_stream as player_stream, restate as player_restate, \
    same_frames
from test_gpu_stream_tools import bits as f64_bits, informer, migrator, random_stream as stream_stream, \
    restate_info, restate_migration
from test_gpu_viz_player import play as viz_play, restate as viz_restate, same as viz_same

pytestmark = pytest.mark.gpu
NONE = 0xFF
PLANES = [(2, 4), (32, 16), (346, 260)]
COUNTS = [1, 1024, 1025, 2600]
CASES = [(w, h, COUNTS[-1]) for w, h in PLANES] + [(32, 16, n) for n in COUNTS[:-1]]
shapes = pytest.mark.parametrize("w,h,n", CASES, ids=[f"{w}x{h}-{n}" for w, h, n in CASES])


def test_the_counts_sit_on_the_sorts_size_edges():
    assert [sort_path(n) for n in COUNTS] == ["block", "block", "merge", "merge"]
    assert COUNTS[1] == BLOCK_SORT_ITEMS and COUNTS[2] == BLOCK_SORT_ITEMS + 1 and COUNTS[3] > 10 * 256
    assert [int(np.ceil(np.log2(w * h + 1))) for w, h in PLANES] == [4, 10, 17]  # keys 0..=units


def rng_of(tool, w, h, n):
    return np.random.default_rng([tool, w, h, n])


def hot_units(rng, w, h, n):
    """unit per record: half of them one of three hot pixels, the others the plane in a shuffled order"""
    units = w * h
    walk = rng.permutation(units)[np.arange(n) % units]
    hot = np.array([0, units // 2, units - 1])[rng.integers(0, 3, n)]
    return np.where(rng.random(n) < 0.5, hot, walk)


def place(ev, u, w):
    ev["x"], ev["y"], ev["c"] = u % w, u // w, NONE
    return ev


# ---- DVS ---------------------------------------------------------------------------------------------------------

@shapes
def test_dvs_convert(w, h, n):
    from adder_amd import dvs
    rng = rng_of(1, w, h, n)
    ev = place(np.zeros(n, S.EVENT_DTYPE), hot_units(rng, w, h, n), w)
    ev["d"] = rng.choice(np.array([0, 1, 2, 3, 5, 7, 8, 9, 12, 20, 40, 127, 128], np.uint8), n)
    ev["t"] = np.where(rng.integers(0, 4, n) == 0, 0, rng.integers(1, 3000, n))
    for time_mode in (0, 1):
        meta = dict(width=w, height=h, channels=1, time_mode=time_mode, ref_interval=255, source_camera=0)
        want, bad = DR.DvsRestatement.from_meta(meta, 0.01).run(ev)
        assert bad is None and (n == 1 or len(want) > 0)
        hd = dvs.HipDvs(**meta)
        assert as_list(hd.convert(ev, dvs.OUT_EVENTS)) == want and hd.bad_index is None
        hd.reset()
        assert hd.convert(ev, dvs.OUT_DAT).tobytes() == DR.dat_bytes(want)


@shapes
def test_dvs_sort(w, h, n):
    """n records straight into dvs_sort: 32-bit times with many ties, which a stable sort leaves in input order"""
    from adder_amd import dvs
    rng = rng_of(2, w, h, n)
    u = hot_units(rng, w, h, n)
    t = np.where(rng.random(n) < 0.5, rng.integers(0, 40, n), rng.integers(0, 1 << 32, n))
    recs = list(zip(t.tolist(), (u % w).tolist(), (u // w).tolist(), rng.integers(0, 2, n).tolist()))
    dat = np.frombuffer(DR.dat_bytes(recs), dvs.DAT_DTYPE)
    got = dvs.HipDvs(w, h).sort(dat, dvs.OUT_DAT)
    assert got.tobytes() == DR.dat_bytes(DR.reorder(recs))


# ---- the players -------------------------------------------------------------------------------------------------

@shapes
@pytest.mark.parametrize("mode", [0, 1])
def test_player(w, h, n, mode):
    """tps 306 000 at 60 fps: a frame length of 5 100 ticks, so the stream shows tens of frames, not hundreds"""
    rng = rng_of(3 + mode, w, h, n)
    ev = place(player_stream(rng, n, w, h, 1, mode, wrap=False), hot_units(rng, w, h, n), w)
    meta = meta_of(w, h, 1, mode, tps=306_000)
    want, final, clock, bad = player_restate(meta, ev, 60.0)
    assert bad is None and len(want) < 100
    hp = make_player(meta, 60.0)
    got = hp.play(ev)
    same_frames(np.concatenate([got, hp.finish().cpu().numpy()]), want)
    assert np.array_equal(bits(hp.display()), bits(final)) and hp.clock() == clock


@shapes
def test_viz_player(w, h, n):
    """A DeltaT stream of viz_player_cases.gen_stream, its records moved to the hot pixels and the walk: in DeltaT any
    t is valid for any unit.  The camera is the DVS one (no round-up) and a hot pixel's steps are short, so that a hot
    pixel does not run a frame ahead per event: the streams pop at most 308 frames."""
    rng = rng_of(5, w, h, n)
    cfg = VK.base_cfg(w, h, 1, time_mode=VK.DELTA_T, source_camera=VK.DVS, buffer_limit=2)
    u = hot_units(rng, w, h, n)
    ev = place(VK.gen_stream(int(rng.integers(1 << 30)), w, h, 1, n), u, w)
    is_hot = np.isin(u, [0, w * h // 2, w * h - 1])
    ev["t"] = np.where(is_hot, rng.integers(1, 12, n), ev["t"])
    r, _ = viz_restate(cfg, ev)
    assert (n == 1 or len(r.popped) > 0) and len(r.popped) < 1024  # the ring viz_play gives the player holds them
    viz_same(viz_play(cfg, ev, form="popped", device=True), r.popped, "popped")
    viz_same(viz_play(cfg, ev, form="running"), r.popped, "running")


# ---- stream tools ------------------------------------------------------------------------------------------------

def stream_meta(w, h, time_mode):
    return dict(width=w, height=h, channels=1, version=2, time_mode=time_mode, ref_interval=255, source_camera=0,
                tps=7650, delta_t_max=7650, adu_interval=0)


@shapes
@pytest.mark.parametrize("time_mode", [0, 1], ids=["forward", "inverse"])
def test_stream_migrate(w, h, n, time_mode):
    rng = rng_of(6 + time_mode, w, h, n)
    ev = stream_stream(rng, n, w, h, 1, time_mode == 1, big_t=False)  # three hot units and the rest of the plane
    meta = stream_meta(w, h, time_mode)
    out_mode = SR.ABSOLUTE_T if time_mode == 0 else SR.DELTA_T
    want, bad = restate_migration(meta, ev, out_mode)
    assert bad is None and len(want) == n
    assert np.array_equal(migrator(meta, out_mode).migrate(ev), want)


@shapes
def test_stream_info_absolute_t(w, h, n):
    rng = rng_of(8, w, h, n)
    ev = stream_stream(rng, n, w, h, 1, True, big_t=False)
    meta = stream_meta(w, h, 1)
    want, bad = restate_info(meta, ev)
    assert bad is None
    got = informer(meta).fold(ev)
    assert (f64_bits(got[0]), f64_bits(got[1]), got[2]) == (f64_bits(want.min), f64_bits(want.max), want.count)


# ---- the framer's feature pass -----------------------------------------------------------------------------------

@shapes
def test_framer_features(w, h, n):
    rng = rng_of(9, w, h, n)
    ev = place(np.zeros(n, FR.EVENT_DTYPE), hot_units(rng, w, h, n), w)
    ev["d"], ev["t"] = rng.integers(0, 9, n), rng.integers(1, 3 * 255, n)
    params = dict(FK.BASE, width=w, height=h)
    ops = [("detect", True), ("ingest", ev)]
    want = FK.run(FR.Restatement(**params), ops)
    got = FK.run(Dev(params, "device"), ops)
    assert (len(want["features"][0]) > 0) == (min(w, h) > 6 and n > 1), "the ring needs 3 pixels to every border"
    assert got["features"] == want["features"]
    assert np.array_equal(got["plane"], want["plane"])
