"""Feature detection while framing on the GPU (include/adder_framer.h, adder_framer_detect_features) against the Python
restatement of Framer::ingest_event (tests/framer_features_oracle.py): features record for record in order, the
running-intensities plane byte for byte, pop_features interval for interval, and the popped frames equal to those of
the same stream ingested with detection off.  Every parity case asserts that the restatement found features."""
import numpy as np
import pytest

from oracle import oracle as O
import clips
import framer_features_cases as K
import framer_features_oracle as R

pytestmark = pytest.mark.gpu

SCENE = dict(tps=7650, ref_interval=255, delta_t_max=510, output_fps=30.0)


def _hip():
    import adder_amd
    return adder_amd


class Dev:
    """HipFramer behind the interface framer_features_cases.run drives"""

    def __init__(self, params, entry="host"):
        A = _hip()
        p = dict(params)
        self.fr = A.HipFramer(p.pop("width"), p.pop("height"), p.pop("channels"), **p)
        self.entry = entry
        self.value_type_log2 = params.get("value_type", 0)
        self.detect = False

    def detect_features(self, on):
        self.fr.detect_features(on)
        self.detect = on

    def reset_last_event(self):
        self.fr.reset_last_event()

    def ingest(self, events):
        import torch
        events = np.ascontiguousarray(events, R.EVENT_DTYPE)
        if self.entry == "host" or not self.detect or not len(events):
            self.fr.ingest(events)  # (its default segments: any stream is safe with detection off)
        else:
            d = torch.from_numpy(events.view(np.uint8).copy()).cuda()
            st = torch.cuda.current_stream().cuda_stream
            # three segments of the one range: with detection on only its two ends count
            offs = np.array([0, len(events) // 3, len(events) // 2, len(events)], np.uint64)
            if self.entry == "device":
                self.fr.ingest_device(d, offs, stream=st)
            elif self.entry == "frames":
                self.fr.ingest_frames_device(d, offs, stream=st)
            else:
                d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
                self.fr.ingest_frames_device_offsets(d, d_offs, 3, stream=st)
            got = self.fr.features()  # waits for the call: `d` may go
            return got
        return self.fr.features() if self.detect else np.zeros(0, R.FEATURE_DTYPE)

    def pop(self):
        return self.fr.pop()

    def write_frame_bytes(self):
        return self.fr.write_frame_bytes()

    def pop_features(self):
        A = _hip()
        try:
            return self.fr.pop_features()
        except A.AdderHipError as e:
            if e.code == A.E_BAD_PARAMS:
                raise R.DequeBroken(str(e))
            raise

    def running_intensities(self):
        return self.fr.running_intensities()


def _check(params, ops, entry="host", min_features=1):
    want = K.run(R.Restatement(**params), ops)
    got = K.run(Dev(params, entry), ops)
    n = sum(len(f) for f in want["features"])
    print(f"restatement: {n} features in {len(want['features'])} calls, {len(want['pops'])} intervals popped")
    assert n >= min_features, "the restatement found no feature: the case shows nothing"
    assert len(got["features"]) == len(want["features"])
    for k, (g, w) in enumerate(zip(got["features"], want["features"])):
        assert g == w, f"features of call {k}"
    assert np.array_equal(got["plane"], want["plane"])
    assert got["pops"] == want["pops"]
    assert got["frames"] == want["frames"]
    # framing itself is untouched: the same calls with detection off pop the same frames
    plain = K.run(Dev(params, "host"), [op if op[0] != "pop_with_features" else ("pop", None) for op in ops
                                        if op[0] in ("ingest", "pop", "write_frame", "pop_with_features")])
    assert plain["frames"] == got["frames"]
    assert not plain["plane"].any()
    return n


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_known_answers(case, entry):
    got = K.run(Dev(case["params"], entry), case["ops"])
    want = K.run(R.Restatement(**case["params"]), case["ops"])
    assert got["features"] == case["features"] == want["features"]
    assert got["pops"] == case["pops"] == want["pops"]
    assert np.array_equal(got["plane"], want["plane"])
    assert got["frames"] == want["frames"]


def _scene_clip(W, H, channels, T):
    return O.synth_clip(O.CONTENT_SCENE, W, H, channels, T).reshape(T, H, W, channels)


def _scene_ops(W, H, channels, time_mode, multi_mode, crf, T=10, per_call=3):
    frames = R.transcode(_scene_clip(W, H, channels, T), time_mode=time_mode, multi_mode=multi_mode, crf=crf,
                         delta_t_max=510)
    ops = [("detect", True)]
    for k in range(0, T, per_call):
        # the player pops an interval per frame; frames are taken as they are (write_frame_bytes), two per three ingested
        ops += [("ingest", np.concatenate(frames[k:k + per_call])), ("pop", None), ("write_frame", 2), ("pop_features", 2)]
    return ops + [("pop_features", 4)]


# number of features the restatement finds in the 160 x 96 cases (fixed on the CPU when the test was written)
SCENE_160_FEATURES = {
    (1, 0, 0, 1): 568,
    (1, 0, 0, 0): 568,
    (1, 0, 3, 1): 557,
    (1, 0, 3, 0): 557,
    (1, 1, 0, 1): 577,
    (1, 1, 0, 0): 577,
    (1, 1, 3, 1): 566,
    (1, 1, 3, 0): 566,
    (3, 0, 0, 1): 571,
    (3, 0, 0, 0): 571,
    (3, 0, 3, 1): 563,
    (3, 0, 3, 0): 563,
    (3, 1, 0, 1): 577,
    (3, 1, 0, 0): 577,
    (3, 1, 3, 1): 569,
    (3, 1, 3, 0): 569,
}


@pytest.mark.parametrize("multi_mode", [O.COLLAPSE, O.NORMAL])
@pytest.mark.parametrize("crf", [0, 3])
@pytest.mark.parametrize("time_mode", [O.DELTA_T, O.ABSOLUTE_T])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("W,H", [(64, 48), (160, 96)])
def test_scene_streams(W, H, channels, time_mode, crf, multi_mode):
    params = dict(SCENE, width=W, height=H, channels=channels, codec_version=2, time_mode=time_mode)
    n = _check(params, _scene_ops(W, H, channels, time_mode, multi_mode, crf), entry="device")
    if W == 160:
        assert n == SCENE_160_FEATURES[(channels, time_mode, crf, multi_mode)]


def _corner_events(channels, time_mode, T=16, seed=5, W=40, H=30):
    clip = clips.make_clip("corners", T, H, W, channels, seed=seed)
    return np.concatenate(R.transcode(clip, time_mode=time_mode, multi_mode=O.COLLAPSE, crf=0, delta_t_max=510))


# (value_type, view_mode, source_type, practical_d_max, delta_t_max): the wider frame types saturate `as u8` at 255, so
# their D / DeltaT views get a divisor that leaves the plane some contrast (a plane that is 255 everywhere has no corner;
# such combinations were replaced when the test was written, the restatement finds nothing in them)
FRAME_CASES = [(0, 0, 0, 12.0, 510), (1, 0, 1, 12.0, 510), (2, 0, 2, 12.0, 510), (0, 1, 0, 12.0, 510),
               (1, 1, 0, 12.0 * 257, 510), (2, 1, 0, 12.0 * 16843009, 510), (0, 2, 0, 12.0, 510),
               (1, 2, 0, 12.0, 510 * 257), (0, 3, 0, 12.0, 510)]


@pytest.mark.parametrize("value_type,view_mode,source_type,practical_d_max,delta_t_max", FRAME_CASES)
@pytest.mark.parametrize("time_mode", [O.DELTA_T, O.ABSOLUTE_T])
def test_frame_types_and_views(value_type, view_mode, source_type, practical_d_max, delta_t_max, time_mode):
    """u8 / u16 / u32 frames (`as u8` of the wider intensities saturates) and the D / DeltaT / SAE views"""
    ev = _corner_events(1, time_mode)
    params = dict(SCENE, width=40, height=30, channels=1, codec_version=2, time_mode=time_mode, value_type=value_type,
                  view_mode=view_mode, source_type=source_type, practical_d_max=practical_d_max, delta_t_max=delta_t_max)
    half = len(ev) // 2
    _check(params, [("detect", True), ("ingest", ev[:half]), ("pop", None), ("ingest", ev[half:]), ("pop", None),
                    ("pop_features", 6)], entry="device")


def _random_stream(rng, n, W, H, channels, time_mode, t_hi):
    ev = np.zeros(n, R.EVENT_DTYPE)
    # a few hot spots: ring pixels and candidates meet often
    ev["x"] = np.clip(rng.integers(0, W, n) // 2 + rng.integers(0, W // 2 + 1, n), 0, W - 1)
    ev["y"] = np.clip(rng.integers(0, H, n) // 2 + rng.integers(0, H // 2 + 1, n), 0, H - 1)
    c = rng.integers(0, channels, n)
    ev["c"] = np.where((channels == 1) & (rng.random(n) < 0.5), 0xFF, c)
    ev["d"] = np.where(rng.random(n) < 0.1, 255, rng.integers(0, 14, n))
    if time_mode == O.ABSOLUTE_T and t_hi:  # 2^d / t with t near 2^32: d 24..35 keeps some contrast in the plane
        ev["d"] = np.where(ev["d"] == 255, 255, ev["d"] + 22)
    if time_mode == O.ABSOLUTE_T:  # mostly rising, with events from the pixels' past and repeated times
        t = np.cumsum(rng.integers(0, 40, n)).astype(np.int64) + 1
        back = rng.random(n) < 0.15
        t = np.where(back, np.maximum(t - rng.integers(0, 3000, n), 1), t)
        if t_hi:
            t = t + (2 ** 32 - 1 - t.max())
    else:
        t = rng.choice(np.array([1, 30, 255, 255, 256, 510, 700, 4000]), n)
        if t_hi:
            t = np.where(rng.random(n) < 0.02, 2 ** 32 - 1 - rng.integers(0, 5, n), t)
    ev["t"] = t
    return ev


@pytest.mark.parametrize("t_hi", [False, True])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("time_mode", [O.DELTA_T, O.ABSOLUTE_T])
def test_random_streams_and_batch_splits(time_mode, channels, t_hi):
    """D_EMPTY, events from the past, t near 2^32 (tps 2^31 -> tpf 2^26: the deque stays small), any order of pixels;
    then the same stream in random batches with empty ones, no pop in between: one call's features, indices shifted."""
    rng = np.random.default_rng(100 * time_mode + 10 * channels + t_hi)
    W, H, n = 24, 20, 6000
    ev = _random_stream(rng, n, W, H, channels, time_mode, t_hi)
    params = dict(width=W, height=H, channels=channels, tps=2 ** 31 if t_hi else 7650, ref_interval=255,
                  delta_t_max=7650, output_fps=32.0 if t_hi else 30.0, codec_version=2, time_mode=time_mode,
                  ring_frames=1 << 12)
    dparams = dict(params)
    params.pop("ring_frames")
    want = R.Restatement(**params)
    want.detect_features(True)
    one = want.ingest(ev)
    assert len(one) > 20
    for entry in ("host", "device", "frames", "frames_offsets"):
        dev = Dev(dparams, entry)
        dev.detect_features(True)
        assert np.array_equal(dev.ingest(ev), one), entry
        assert np.array_equal(dev.running_intensities(), want.running)
    cuts = np.sort(rng.integers(0, n + 1, 9))
    cuts = np.concatenate([[0, 0], cuts, cuts[-1:], [n, n]])
    dev = Dev(dparams, "device")
    dev.detect_features(True)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        f = dev.ingest(ev[int(a):int(b)]).copy()
        f["index"] += np.uint64(int(a))
        parts.append(f)
    assert np.array_equal(np.concatenate(parts), one)
    assert np.array_equal(dev.running_intensities(), want.running)
    for _ in range(4):
        if want.broken:
            with pytest.raises(R.DequeBroken):
                dev.pop_features()
            break
        a, b = want.pop_features(), dev.pop_features()
        assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_pops_resets_and_toggles_between_calls():
    """frames_written changes between calls (pops), last_event is reset, detection goes off and on mid-stream"""
    for time_mode in (O.DELTA_T, O.ABSOLUTE_T):
        ev = _corner_events(3, time_mode, T=20, seed=8)
        q = len(ev) // 6
        params = dict(SCENE, width=40, height=30, channels=3, codec_version=2, time_mode=time_mode)
        ops = [("detect", True), ("ingest", ev[:q]), ("pop_with_features",), ("ingest", ev[q:2 * q]),
               ("reset",), ("ingest", ev[2 * q:3 * q]), ("pop_with_features",), ("detect", False),
               ("ingest", ev[3 * q:4 * q]), ("pop_with_features",), ("detect", True), ("ingest", ev[4 * q:5 * q]),
               ("reset",), ("ingest", ev[5 * q:]), ("pop_with_features",), ("pop_features", 3)]
        for entry in ("host", "device"):
            _check(params, ops, entry=entry, min_features=50)


def test_capacity_error_changes_nothing_and_band_context_is_refused():
    import ctypes as C
    A = _hip()
    case = K.CASES[6]  # two features in one call
    assert case["name"] == "three_pixel_border_rejects"
    dev = Dev(case["params"])
    dev.detect_features(True)
    dev.ingest(K.make_events(case["ops"][1][1]))
    fr = dev.fr
    n = C.c_uint64(0)
    buf = np.zeros(2, A.FRAMER_FEATURE_DTYPE)
    assert fr.L.adder_framer_features(fr.h, buf.ctypes.data, 1, C.byref(n)) == A.E_OUT_CAPACITY
    assert n.value == 2 and not buf["t"].any()
    assert fr.L.adder_framer_features(fr.h, buf.ctypes.data, 2, C.byref(n)) == A.OK
    assert [(int(r["index"]), int(r["t"]), int(r["x"]), int(r["y"])) for r in buf] == case["features"][0]
    end_ts, m = C.c_uint64(0), C.c_uint32(0)
    xy = np.zeros((2, 2), np.uint16)
    assert fr.L.adder_framer_pop_features(fr.h, C.byref(end_ts), xy.ctypes.data, 1, C.byref(m)) == A.E_OUT_CAPACITY
    assert m.value == 2
    assert fr.L.adder_framer_pop_features(fr.h, C.byref(end_ts), xy.ctypes.data, 2, C.byref(m)) == A.OK
    assert end_ts.value == 255 and xy.tolist() == [[3, 4], [5, 5]]  # the refused pop had not moved the deque

    band = A.HipFramer(9, 9, 1, row_begin=3, row_end=9, **{k: v for k, v in K.BASE.items()
                                                          if k not in ("width", "height", "channels")})
    with pytest.raises(A.AdderHipError) as ei:
        band.detect_features(True)
    assert ei.value.code == A.E_BAD_PARAMS
    band.detect_features(False)  # switching it off is always fine


def test_features_and_plane_in_device_memory():
    import torch
    A = _hip()
    ev = _corner_events(1, O.DELTA_T)
    params = dict(SCENE, width=40, height=30, channels=1, codec_version=2, time_mode=O.DELTA_T)
    want = R.Restatement(**params)
    want.detect_features(True)
    one = want.ingest(ev)
    dev = Dev(params, "device")
    dev.detect_features(True)
    assert np.array_equal(dev.ingest(ev), one) and len(one) > 20
    d_feat = torch.zeros((len(one) + 3, 16), dtype=torch.uint8, device="cuda")
    d_plane = torch.zeros(40 * 30, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert dev.fr.features_device(d_feat, stream=st) == len(one)
    dev.fr.running_intensities_device(d_plane, stream=st)
    torch.cuda.synchronize()
    got = np.frombuffer(d_feat.cpu().numpy().tobytes(), A.FRAMER_FEATURE_DTYPE)[: len(one)]
    assert np.array_equal(got, one)
    assert np.array_equal(d_plane.cpu().numpy().reshape(30, 40, 1), want.running)


def test_hd_stream_from_the_device():
    """1920 x 1080 gray x 60 frames of the scene clip, transcoded on the device (DeltaT, crf 0), one ingest_device call.
    The Python restatement is too slow for the whole stream: the C++ mirror (FeatureTracker, the serial loop on the host)
    is compared on ALL of it -- every feature and the whole plane -- and the Python restatement on the events of a
    160 x 96 window (the cell where the mirror found most features), shifted to the origin and re-ingested on their own
    by both the restatement and the device."""
    import ctypes as C
    import torch
    import framer_features_host_py as M
    A = _hip()
    W, H, T = 1920, 1080, 60
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.empty((T, W * H), dtype=torch.uint8, device="cuda")
    A.synth_clip_device(d_frames, A.CONTENT_SCENE, W, H, 1, num_frames=T, stream=st)
    d_ev = torch.empty((int(W * H * T * 0.75) + 1024, 3), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    hv = A.HipVideo(W, H, 1, time_mode=A.TIME_DELTA_T, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=255)
    hv.update_crf(0)
    hv.integrate_device(d_frames, d_ev, d_off, stream=st)
    n = hv.finish()
    torch.cuda.synchronize()
    kw = dict(tps=7650, ref_interval=255, delta_t_max=255, output_fps=30.0, codec_version=2, time_mode=A.TIME_DELTA_T)
    fr = A.HipFramer(W, H, 1, ring_frames=1024, **kw)
    fr.detect_features(True)
    fr.ingest_device(d_ev[:n], [0, n], stream=st)
    got = fr.features()
    plane = fr.running_intensities()
    events = np.frombuffer(d_ev[:n].cpu().numpy().tobytes(), A.EVENT_DTYPE)
    print(f"{n} events, {len(got)} features on the device")

    L = M.lib()
    params = np.array([kw["tps"], 255, 255, 2, A.TIME_DELTA_T, 0, 0, 0, 0], np.uint32)
    h = L.adder_host_features_new(W, H, 1, params.ctypes.data, 30.0, 0.0)
    L.adder_host_features_detect(h, 1)
    lv, lt = C.c_int(0), C.c_uint32(0)
    want = []
    for a in range(0, n, 1 << 22):
        part = np.ascontiguousarray(events[a:a + (1 << 22)])
        out = np.zeros(len(part), A.FRAMER_FEATURE_DTYPE)
        m = L.adder_host_features_ingest(h, part.ctypes.data, len(part), C.byref(lv), C.byref(lt), 0, a, out.ctypes.data)
        want.append(out[:m].copy())
    want = np.concatenate(want)
    mirror_plane = np.zeros((H, W, 1), np.uint8)
    L.adder_host_features_plane(h, mirror_plane.ctypes.data)
    L.adder_host_features_free(h)
    assert len(want) > 1000
    assert np.array_equal(got, want)
    assert np.array_equal(plane, mirror_plane)

    # the window: the 160 x 96 cell of the plane in which the mirror found most features (the scene is flat elsewhere)
    w, hh = 160, 96
    cells = np.bincount((want["y"] // hh).astype(np.int64) * (W // w) + (want["x"] // w).astype(np.int64),
                        minlength=(H // hh + 1) * (W // w))
    x0, y0 = int(cells.argmax() % (W // w)) * w, int(cells.argmax() // (W // w)) * hh
    y0 = min(y0, H - hh)
    inside = (events["x"] >= x0) & (events["x"] < x0 + w) & (events["y"] >= y0) & (events["y"] < y0 + hh)
    crop = events[inside].copy()
    crop["x"] -= x0
    crop["y"] -= y0
    r = R.Restatement(w, hh, 1, **kw)
    r.detect_features(True)
    one = r.ingest(crop)
    assert len(one) > 20
    small = A.HipFramer(w, hh, 1, ring_frames=1024, **kw)
    small.detect_features(True)
    d_crop = torch.from_numpy(crop.view(np.uint8).copy()).cuda()
    small.ingest_device(d_crop, [0, len(crop)], stream=st)
    assert np.array_equal(small.features(), one)
    assert np.array_equal(small.running_intensities(), r.running)
