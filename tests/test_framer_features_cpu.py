"""Feature detection while framing (FrameSequence::detect_features, framer/driver.rs:482-553, 846-873) on the CPU.

The Python restatement (tests/framer_features_oracle.py) is pinned three ways: its intensities against the framer
checker's popped frames, its rules against hand-derived known answers (tests/framer_features_cases.py), and, once
pinned, it is the standard for the C++ mirror and for the device's per-event logic compiled for the host.
"""
import numpy as np
import pytest

from oracle import oracle as O
import clips
import framer_features_cases as K
import framer_features_oracle as R


def _restatement(params):
    return R.Restatement(**params)


@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_known_answers_restatement(case):
    log = K.run(_restatement(case["params"]), case["ops"])
    assert log["features"] == case["features"]
    assert log["pops"] == case["pops"]


def _streams():
    for channels, time_mode, multi_mode, crf, seed in [(1, O.DELTA_T, O.COLLAPSE, 0, 1), (3, O.ABSOLUTE_T, O.NORMAL, 3, 2),
                                                       (1, O.ABSOLUTE_T, O.COLLAPSE, 0, 3), (3, O.DELTA_T, O.NORMAL, 0, 4)]:
        clip = clips.make_clip("corners", 30, 24, 32, channels, seed=seed)
        yield channels, time_mode, np.concatenate(R.transcode(clip, time_mode=time_mode, multi_mode=multi_mode, crf=crf,
                                                              delta_t_max=510))


def test_restatement_frames_equal_the_framer_checker():
    """Every (unit, frame) intensity of the restatement is what oracle.Framer pops for the same stream, with detection
    on: ties val8 (the unit's last frame intensity) to the existing checker."""
    total = 0
    for channels, time_mode, events in _streams():
        kw = dict(tps=7650, ref_interval=255, delta_t_max=510, output_fps=30.0, codec_version=2, time_mode=time_mode)
        of = O.Framer(32, 24, channels, chunk_rows=64, **kw)
        want = of.ingest_events(events) + of.write_multi_frame_bytes()
        r = R.Restatement(32, 24, channels, **kw)
        r.detect_features(True)
        got = b""
        for a in range(0, len(events), 997):
            feats = r.ingest(events[a:a + 997])
            got += r.pop()
            total += len(feats)
        assert len(want) >= 2 * 32 * 24 * channels and got == want
    assert total > 100


def test_restatement_is_batch_invariant_without_pops():
    for channels, time_mode, events in _streams():
        kw = dict(tps=7650, ref_interval=255, delta_t_max=510, output_fps=30.0, codec_version=2, time_mode=time_mode)
        a, b = R.Restatement(32, 24, channels, **kw), R.Restatement(32, 24, channels, **kw)
        a.detect_features(True)
        b.detect_features(True)
        one = a.ingest(events)
        parts, at = [], 0
        for n in (0, 1, 500, 0, 3000, len(events)):
            parts.append(b.ingest(events[at:at + n], index_base=at))
            at += n
        assert len(one) > 0 and np.array_equal(one, np.concatenate(parts))
        assert np.array_equal(a.running, b.running)
        assert list(a.features) == list(b.features)


# ---- the device's per-event logic compiled for the host (tests/cpu_sim/framer_features_sim.cpp) ----

def _compare(make, params, ops, min_features=1):
    want = K.run(_restatement(params), ops)
    got = K.run(make(**params), ops)
    assert sum(len(f) for f in want["features"]) >= min_features
    assert got["features"] == want["features"]
    assert np.array_equal(got["plane"], want["plane"])
    assert got["pops"] == want["pops"]
    assert got["frames"] == want["frames"]


def _stream_ops(events, rng):
    cuts = np.concatenate([[0], np.sort(rng.integers(0, len(events), 5)), [len(events)]])
    ops = [("detect", True)]
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        ops.append(("ingest", events[a:b]))
        if k == 1:
            ops += [("write_frame", 2), ("pop_features", 2)]
        if k == 2:
            ops += [("reset",), ("detect", False)]
        if k == 3:
            ops += [("detect", True), ("pop", None)]
    return ops + [("pop_features", 6)]


def _random_events(rng, n, W, H, channels, abs_t):
    ev = np.zeros(n, R.EVENT_DTYPE)
    ev["x"] = rng.integers(0, W, n)
    ev["y"] = rng.integers(0, H, n)
    ev["c"] = np.where((channels == 1) & (rng.random(n) < 0.5), 0xFF, rng.integers(0, channels, n))
    ev["d"] = np.where(rng.random(n) < 0.1, 255, rng.integers(0, 14, n))
    if abs_t:  # mostly rising, with events from the pixels' past and repeated times
        t = np.cumsum(rng.integers(0, 40, n)).astype(np.int64) + 1
        t = np.where(rng.random(n) < 0.15, np.maximum(t - rng.integers(0, 3000, n), 1), t)
    else:
        t = rng.choice(np.array([1, 30, 255, 255, 256, 510, 700, 4000]), n)
    ev["t"] = t
    return ev


def _sim(**params):
    import framer_features_sim_py
    return framer_features_sim_py.SimFramer(**params)


@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_known_answers_device_logic_on_the_host(case):
    log = K.run(_sim(**case["params"]), case["ops"])
    assert log["features"] == case["features"]
    assert log["pops"] == case["pops"]


def test_device_logic_on_the_host_equals_the_restatement_on_streams():
    rng = np.random.default_rng(5)
    for channels, time_mode, events in _streams():
        params = dict(width=32, height=24, channels=channels, tps=7650, ref_interval=255, delta_t_max=510,
                      output_fps=30.0, codec_version=2, time_mode=time_mode)
        _compare(_sim, params, _stream_ops(events, rng), min_features=30)
    for channels in (1, 3):
        for time_mode in (O.DELTA_T, O.ABSOLUTE_T):
            for value_type, view_mode in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (0, 3), (1, 2)):
                params = dict(width=16, height=14, channels=channels, tps=7650, ref_interval=255, delta_t_max=7650,
                              output_fps=30.0, codec_version=2, time_mode=time_mode, value_type=value_type,
                              view_mode=view_mode, practical_d_max=12.0)
                ev = _random_events(rng, 3000, 16, 14, channels, time_mode == O.ABSOLUTE_T)
                _compare(_sim, params, _stream_ops(ev, rng), min_features=5)


def test_ring_form_of_the_corner_test_equals_the_literal_scan():
    import framer_features_sim_py
    import framer_features_images
    positives = 0
    for img in framer_features_images.images():
        L = O.lib()
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        want = np.array([[L.oracle_fast_is_feature(img.ctypes.data, w, h, ch, x, y) for x in range(w)] for y in range(h)],
                        np.uint8).reshape(h, w)
        assert np.array_equal(framer_features_sim_py.fast9_ring16_plane(img), want)
        positives += int(want.sum())
    assert positives > 200


# ---- the C++ mirror (adder-codec-rs_amd/host: FeatureTracker, the reference's serial loop on the host) ----

def _mirror(**params):
    import framer_features_host_py
    return framer_features_host_py.MirrorFramer(**params)


@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_known_answers_cpp_mirror(case):
    log = K.run(_mirror(**case["params"]), case["ops"])
    assert log["features"] == case["features"]
    assert log["pops"] == case["pops"]


def test_cpp_mirror_equals_the_restatement_on_streams():
    rng = np.random.default_rng(6)
    for channels, time_mode, events in _streams():
        params = dict(width=32, height=24, channels=channels, tps=7650, ref_interval=255, delta_t_max=510,
                      output_fps=30.0, codec_version=2, time_mode=time_mode)
        _compare(_mirror, params, _stream_ops(events, rng), min_features=30)
    for channels in (1, 3):
        for time_mode in (O.DELTA_T, O.ABSOLUTE_T):
            for value_type, view_mode in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (0, 3), (1, 2)):
                params = dict(width=16, height=14, channels=channels, tps=7650, ref_interval=255, delta_t_max=7650,
                              output_fps=30.0, codec_version=2, time_mode=time_mode, value_type=value_type,
                              view_mode=view_mode, practical_d_max=12.0)
                ev = _random_events(rng, 3000, 16, 14, channels, time_mode == O.ABSOLUTE_T)
                _compare(_mirror, params, _stream_ops(ev, rng), min_features=5)
