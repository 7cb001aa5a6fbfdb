"""The dense FAST detector and the feature scores on the device (include/adder_fast.h, adder_amd.HipFastEval) against
the definition in tests/fast_eval_oracle.py, every pixel compared: planes without and with one candidate, every byte
phase of the row-end stores (widths 61..67, one each side of the tile's width and height), frame independence, three
channels with decoys, thresholds 1 / 30 / 255, suppression on and off, a large plane, each output left out in turn,
a coordinate list one too short, mask_from_xy, every prediction case, the transcoder's planes end to end, and the host
forms."""
import math

import numpy as np
import pytest

import fast_eval_cases as K
import fast_eval_oracle as O

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 128, 32   # csrc/adder_fast_kernels.h kFastTileW, kFastTileH
GUARD = 0xA5


def _hip():
    import adder_amd
    return adder_amd


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SCORES = {}


def want(key, frames, threshold, nonmax):
    """The oracle's (mask, score, xy, counts) of a plane set; the scores are computed once per (key, threshold) and
    serve both settings of the suppression."""
    k = (key, threshold)
    if k not in _SCORES:
        _SCORES[k] = [O.score_plane(f, threshold) for f in frames]
    return O.stack([O.from_score(s, nonmax) for s in _SCORES[k]])


def run_device(frames, threshold, nonmax, channels=1):
    """frames [n][H][W] or [n][H][W][3] -> (mask, score, xy, counts) from one detect_device call, with guard bytes
    around every output checked."""
    import torch
    A = _hip()
    n, h, w = frames.shape[:3]
    fe = A.HipFastEval(w, h, channels, threshold=threshold, nonmax=nonmax)
    plane = n * h * w
    pad = 64 + h % 4   # (the outputs' first byte off a dword for most heights)
    mask = torch.full((plane + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    score = torch.full((plane + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    xy = torch.full((plane + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    counts = fe.detect_device(_cuda(frames), mask[pad:pad + plane], score[pad:pad + plane], xy[pad:pad + plane])
    fe.close()
    mask, score, xy = mask.cpu().numpy(), score.cpu().numpy(), xy.cpu().numpy().view(np.uint32)
    total = int(counts.sum())
    for buf in (mask, score):
        assert (buf[:pad] == GUARD).all() and (buf[pad + plane:] == GUARD).all()
    assert (xy[:pad] == 0x5A5A5A5A).all() and (xy[pad + total:] == 0x5A5A5A5A).all()
    return (mask[pad:pad + plane].reshape(n, h, w), score[pad:pad + plane].reshape(n, h, w), xy[pad:pad + total], counts)


def check(key, frames, threshold, nonmax, channels=1, planes=None):
    """planes: the [n][H][W] planes the oracle sees when `frames` carries decoy channels."""
    w_mask, w_score, w_xy, w_counts = want(key, frames if planes is None else planes, threshold, nonmax)
    mask, score, xy, counts = run_device(frames, threshold, nonmax, channels)
    assert np.array_equal(score, w_score)
    assert np.array_equal(mask, w_mask)
    assert np.array_equal(counts, w_counts)
    assert np.array_equal(xy, w_xy)


@pytest.mark.parametrize("nonmax", (False, True))
@pytest.mark.parametrize("shape", ((7, 7), (6, 9), (9, 6)))
def test_smallest_planes(shape, nonmax):
    w, h = shape
    name = {(7, 7): "one_candidate_7x7", (6, 9): "no_candidates_6x9", (9, 6): "no_candidates_9x6"}[shape]
    frames = K.CASES[name].frames
    assert frames.shape[1:] == (h, w)
    check(name, frames, 30, nonmax)
    if shape != (7, 7):  # no candidates: zero key points, all true negatives
        A = _hip()
        fe = A.HipFastEval(w, h, threshold=30, nonmax=nonmax)
        ev = fe.evaluate_device(_cuda(frames), _cuda(np.zeros((1, h, w), np.uint8)))[0]
        assert (ev["gt_count"], ev["tp"], ev["fp"], ev["fn"], ev["tn"]) == (0, 0, 0, 0, w * h)
        assert math.isnan(ev["precision"]) and math.isnan(ev["recall"]) and ev["accuracy"] == 1.0
        fe.close()


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_cases(name):
    case = K.CASES[name]
    for threshold in case.thresholds:
        for nonmax in (False, True):
            check(name, case.frames, threshold, nonmax)


@pytest.mark.parametrize("w", (61, 62, 63, 64, 65, 66, 67, TILE_W - 1, TILE_W, TILE_W + 1))
def test_widths(w):
    """Every byte phase of a row's start and end in the planes (three frames of odd height: the frames' starts take every
    phase too), rings and 3x3 neighbourhoods across a tile seam in x."""
    frames = K.noise_and_squares(w, 37, 100 + w, n=3)
    for nonmax in (False, True):
        check(("w", w), frames, 30, nonmax)


@pytest.mark.parametrize("h", (TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1))
def test_heights(h):
    frames = K.noise_and_squares(131, h, 200 + h)
    for nonmax in (False, True):
        check(("h", h), frames, 30, nonmax)


def test_frames_are_independent():
    frames = np.concatenate([K.noise(67, 45, 31), K.squares(67, 45, 32), K.noise_and_squares(67, 45, 33)])
    for nonmax in (False, True):
        together = run_device(frames, 30, nonmax)
        for k in range(3):
            alone = run_device(frames[k:k + 1], 30, nonmax)
            assert np.array_equal(together[0][k], alone[0][0]) and np.array_equal(together[1][k], alone[1][0])
            assert together[3][k] == alone[3][0]
        check("independent", frames, 30, nonmax)


@pytest.mark.parametrize("w", (65, 130))
def test_three_channels_with_decoys(w):
    planes = K.noise_and_squares(w, 35, 300 + w, n=2)
    decoy = K.noise(w, 35, 301 + w, n=4).reshape(2, 2, 35, w)
    frames = np.stack([planes, decoy[:, 0], decoy[:, 1]], axis=-1)
    for nonmax in (False, True):
        check(("c3", w), frames, 30, nonmax, channels=3, planes=planes)


@pytest.mark.parametrize("threshold", (1, 30, 255))
def test_thresholds(threshold):
    frames = K.noise(133, 35, 40)
    for nonmax in (False, True):
        check("thresholds", frames, threshold, nonmax)


def test_large_plane():
    frames = K.noise_and_squares(1283, 725, 50)
    check("large", frames, 30, True)
    check("large", frames, 30, False)


@pytest.mark.parametrize("nonmax", (False, True))
def test_each_output_left_out(nonmax):
    import torch
    A = _hip()
    frames = K.noise_and_squares(131, 35, 60, n=2)
    n, h, w = frames.shape
    w_mask, w_score, w_xy, w_counts = want("left_out", frames, 30, nonmax)
    fe = A.HipFastEval(w, h, threshold=30, nonmax=nonmax)
    d = _cuda(frames)
    for skip in ("mask", "score", "xy", "all"):
        mask = None if skip in ("mask", "all") else torch.zeros(n * h * w, dtype=torch.uint8, device="cuda")
        score = None if skip in ("score", "all") else torch.zeros(n * h * w, dtype=torch.uint8, device="cuda")
        xy = None if skip in ("xy", "all") else torch.zeros(len(w_xy), dtype=torch.int32, device="cuda")
        counts = fe.detect_device(d, mask, score, xy)
        assert np.array_equal(counts, w_counts), skip
        if mask is not None:
            assert np.array_equal(mask.cpu().numpy().reshape(n, h, w), w_mask), skip
        if score is not None:
            assert np.array_equal(score.cpu().numpy().reshape(n, h, w), w_score), skip
        if xy is not None:
            assert np.array_equal(xy.cpu().numpy().view(np.uint32), w_xy), skip
    fe.close()


def test_capacity_one_short():
    import torch
    A = _hip()
    frames = K.noise_and_squares(131, 35, 61, n=2)
    n, h, w = frames.shape
    w_mask, _, w_xy, w_counts = want("capacity", frames, 30, False)
    assert len(w_xy) > 8
    fe = A.HipFastEval(w, h, threshold=30)
    pad = 16
    buf = torch.full((len(w_xy) - 1 + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    mask = torch.zeros(n * h * w, dtype=torch.uint8, device="cuda")
    with pytest.raises(A.AdderHipError) as ei:
        fe.detect_device(_cuda(frames), mask, None, buf[pad:pad + len(w_xy) - 1])
    assert ei.value.code == A.E_OUT_CAPACITY
    assert np.array_equal(ei.value.counts, w_counts)
    assert (buf.cpu().numpy() == 0x5A5A5A5A).all()           # nothing written, the guards untouched
    assert np.array_equal(mask.cpu().numpy().reshape(n, h, w), w_mask)
    # the context goes on: an exact fit
    exact = torch.zeros(len(w_xy), dtype=torch.int32, device="cuda")
    assert np.array_equal(fe.detect_device(_cuda(frames), None, None, exact), w_counts)
    assert np.array_equal(exact.cpu().numpy().view(np.uint32), w_xy)
    fe.close()


def test_mask_from_xy():
    import torch
    A = _hip()
    w, h = 67, 21
    fe = A.HipFastEval(w, h)
    pts = [(0, 0), (66, 20), (5, 7), (5, 7), (66, 0), (0, 20), (5, 7), (33, 9)]   # with duplicates
    xy = np.array([x | (y << 16) for x, y in pts], np.uint32)
    expect = np.zeros((h, w), np.uint8)
    for x, y in pts:
        expect[y, x] = 1
    mask = torch.full((h * w + 32,), GUARD, dtype=torch.uint8, device="cuda")
    fe.mask_from_xy(_cuda(xy.view(np.int32)), mask[16:16 + h * w])
    got = mask.cpu().numpy()
    assert np.array_equal(got[16:16 + h * w].reshape(h, w), expect)
    assert (got[:16] == GUARD).all() and (got[16 + h * w:] == GUARD).all()
    # one coordinate outside the plane (x = W; y = H): refused, and no write at all
    for bad in (w | (3 << 16), 3 | (h << 16)):
        mask.fill_(GUARD)
        with pytest.raises(A.AdderHipError) as ei:
            fe.mask_from_xy(_cuda(np.append(xy, np.uint32(bad)).view(np.int32)), mask[16:16 + h * w])
        assert ei.value.code == A.E_BAD_PARAMS
        assert (mask.cpu().numpy() == GUARD).all()
    # an empty list clears the plane
    fe.mask_from_xy(torch.zeros(0, dtype=torch.int32, device="cuda"), mask[16:16 + h * w])
    assert not mask[16:16 + h * w].any().item()
    # a list the detector made scores 1 / 1 / 1 against the detector
    frames = K.squares(w, h, 70)
    out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    n = int(fe.detect_device(_cuda(frames), None, None, out)[0])
    assert n > 0
    ev = fe.evaluate_device(_cuda(frames), fe.mask_from_xy(out[:n]))[0]
    assert (ev["tp"], ev["fp"], ev["fn"]) == (n, 0, 0) and ev["precision"] == ev["recall"] == ev["accuracy"] == 1.0
    fe.close()


def _same(a, b):
    return a == b or (a != a and b != b)


def _check_eval(got, gt_mask, pred):
    w = O.precision_recall_accuracy(gt_mask, pred)
    for k in ("tp", "fp", "tn", "fn", "gt_count", "pred_count"):
        assert got[k] == w[k], (k, got, w)
    for k in ("precision", "recall", "accuracy"):
        assert _same(got[k], w[k]), (k, got, w)
    return w


@pytest.mark.parametrize("nonmax", (False, True))
def test_evaluate_every_prediction_case(nonmax):
    """Empty, full, equal to the truth, disjoint from it and mixed, on a busy plane, a constant one (0 / 0 twice) and one
    whose W * H is odd (the second frame's planes start off a dword), all in one three-frame call."""
    A = _hip()
    w, h = 67, 45
    frames = np.concatenate([K.noise_and_squares(w, h, 80), np.full((1, h, w), 9, np.uint8), K.squares(w, h, 81)])
    truth = want(("eval", w), frames, 30, nonmax)[0]
    preds = [K.predictions(t, seed=90 + i) for i, t in enumerate(truth)]
    fe = A.HipFastEval(w, h, threshold=30, nonmax=nonmax)
    d = _cuda(frames)
    seen_nan = False
    for pname in preds[0]:
        pred = np.stack([p[pname] for p in preds])
        got = fe.evaluate_device(d, _cuda(pred))
        host = fe.evaluate(frames, pred)
        for k in range(3):
            ev = _check_eval(got[k], truth[k], pred[k])
            assert all(_same(got[k][key], host[k][key]) for key in got[k])
            seen_nan |= ev["precision"] != ev["precision"] and ev["recall"] != ev["recall"] and ev["accuracy"] == 1.0
    assert seen_nan
    fe.close()


def test_end_to_end_with_the_transcoder():
    """A moving square through HipVideo with detection on: after every frame the membership plane's device copy equals
    the host copy, and evaluate_device on the two device planes equals the oracle on host copies."""
    import torch
    A = _hip()
    W, H, T = 64, 48, 6
    clip = np.full((T, H, W), 30, np.uint8)
    for f in range(T):
        clip[f, 8 + 3 * f:20 + 3 * f, 10 + 5 * f:24 + 5 * f] = 150 + 6 * np.add.outer(np.arange(12), np.arange(14))
    hv = A.HipVideo(W, H, 1, time_mode=A.TIME_ABSOLUTE_T, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=7650)
    hv.set_crf_parameters(7, 7)
    hv.reset_c_thresh(2)
    hv.update_detect_features(True, False)
    assert not hv.feature_set_device().any().item()          # before any frame: all zeros
    fe = A.HipFastEval(W, H, threshold=30, nonmax=False)
    fe_nm = A.HipFastEval(W, H, threshold=30, nonmax=True)
    d_plane = torch.zeros(H * W, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    features_seen = 0
    for f in range(T):
        hv.integrate_matrix(clip[f])
        host_set = hv.feature_set()
        d_set = hv.feature_set_device(stream=stream)
        assert np.array_equal(d_set.cpu().numpy(), host_set), f
        hv.running_intensities_device(d_plane, stream=stream)
        plane = hv.running_intensities().reshape(H, W)
        assert np.array_equal(d_plane.cpu().numpy().reshape(H, W), plane), f
        for e, nonmax in ((fe, False), (fe_nm, True)):
            got = e.evaluate_device(d_plane, d_set, stream=stream)[0]
            _check_eval(got, O.detect(plane, 30, nonmax)[0], host_set)
        features_seen = max(features_seen, int(host_set.sum()))
    assert features_seen > 0
    fe.close()
    fe_nm.close()
    hv.close()


@pytest.mark.parametrize("channels", (1, 3))
def test_host_forms_equal_the_device_forms(channels):
    A = _hip()
    planes = K.noise_and_squares(131, 35, 95, n=2)
    frames = planes if channels == 1 else np.stack([planes, 255 - planes, planes // 2], axis=-1)
    for nonmax in (False, True):
        dev = run_device(frames, 30, nonmax, channels)
        fe = A.HipFastEval(131, 35, channels, threshold=30, nonmax=nonmax)
        host = fe.detect(frames, mask=True, score=True, xy=True)
        assert np.array_equal(host["mask"], dev[0]) and np.array_equal(host["score"], dev[1])
        assert np.array_equal(host["xy"], dev[2]) and np.array_equal(host["counts"], dev[3])
        only_counts = fe.detect(frames, mask=False)
        assert np.array_equal(only_counts["counts"], dev[3]) and only_counts["mask"] is None
        with pytest.raises(A.AdderHipError) as ei:
            fe.detect(frames, xy=True, capacity=int(dev[3].sum()) - 1)
        assert ei.value.code == A.E_OUT_CAPACITY and np.array_equal(ei.value.counts, dev[3])
        assert np.array_equal(ei.value.mask, dev[0])
        fe.close()


def test_refusals():
    A = _hip()
    for kw in (dict(threshold=0), dict(channels=2), dict(width=0)):
        args = dict(width=16, height=16, channels=1, threshold=30)
        args.update(kw)
        with pytest.raises(A.AdderHipError) as ei:
            A.HipFastEval(args.pop("width"), args.pop("height"), args.pop("channels"), **args)
        assert ei.value.code == A.E_BAD_PARAMS
