"""Quality metrics on the device (include/adder_quality.h): MSE / PSNR against the host mirror bit for bit, every
SSIM window against the restatement of cv.rs (tests/quality_oracle.py) bit for bit, the frame's SSIM within the
bound of the summation orders, determinism, the transcoder -> framer -> metrics chain and the viewer's running plane
on one stream, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import oracle as O
import quality_oracle as Q

pytestmark = pytest.mark.gpu


def _hip():
    import adder_amd
    return adder_amd


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_frames(A, a, b, got, dmap=None, check_ssim=True):
    """a, b: [n][H][W][C] uint8; got: the device's dicts; dmap: the device's map [n][C][H-7][W-7]."""
    n, H, W, Cn = a.shape
    for k in range(n):
        assert {"mse": got[k]["mse"], "psnr": got[k]["psnr"]} == A.calculate_quality_metrics(a[k], b[k]), k
        if not check_ssim:
            continue
        s, m, _, abs_sums, terms = Q.fast_ssim(a[k], b[k], want_map=dmap is not None)
        if H < 8 or W < 8:
            assert math.isnan(got[k]["ssim"])
            continue
        if dmap is not None:
            assert (bits(dmap[k]) == bits(m)).all(), k
        d = got[k]["ssim"]
        nwin = (H - 7) * (W - 7)
        assert abs(d - s) <= Q.ssim_bound(abs_sums, Cn), (k, d, s)
        assert abs(d - Q.fsum_ssim(terms, nwin)) <= Q.fsum_bound(abs_sums, Cn, nwin), (k, d)


def test_random_shapes_against_the_restatement():
    import torch
    A = _hip()
    rng = np.random.default_rng(2024)
    for case in range(14):
        H, W = int(rng.integers(8, 68)), int(rng.integers(8, 42))
        Cn = int(rng.choice([1, 3]))
        n = int(rng.integers(1, 8))
        a = rng.integers(0, 256, (n, H, W, Cn), dtype=np.uint8)
        kind = case % 3
        if kind == 0:
            b = np.clip(a.astype(np.int16) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
        elif kind == 1:
            b = rng.integers(0, 256, a.shape, dtype=np.uint8)
        else:
            b = 255 - a
        q = A.HipQuality(W, H, Cn, ssim=True)
        dmap = torch.full(q.map_shape(n), -7.0, dtype=torch.float64, device="cuda")
        got = q.compute_device(_cuda(a), _cuda(b), ssim_map=dmap)
        _check_frames(A, a, b, got, dmap.cpu().numpy())
        # the host-pointer form: the same numbers and map
        hmap = np.full(q.map_shape(n), -7.0)
        host = q.compute(a, b, ssim_map=hmap)
        assert [bits(list(g.values())).tolist() for g in host] == [bits(list(g.values())).tolist() for g in got]
        assert (bits(hmap) == bits(dmap.cpu().numpy())).all()


def test_known_answers_on_the_device():
    A = _hip()
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (2, 33, 17, 3), dtype=np.uint8)
    got = A.HipQuality(17, 33, 3, ssim=True).compute_device(_cuda(a), _cuda(a))
    for g in got:
        assert g == {"mse": 1e-7, "psnr": 20.0 * math.log10(255.0) + 70.0, "ssim": 100.0}
    for H, W in ((7, 20), (20, 5)):
        a = rng.integers(0, 256, (3, H, W, 1), dtype=np.uint8)
        b = rng.integers(0, 256, (3, H, W, 1), dtype=np.uint8)
        got = A.HipQuality(W, H, 1, ssim=True).compute_device(_cuda(a), _cuda(b))
        for k, g in enumerate(got):
            assert math.isnan(g["ssim"])
            assert {"mse": g["mse"], "psnr": g["psnr"]} == A.calculate_quality_metrics(a[k], b[k])
    # the mask: only what is asked for
    q = A.HipQuality(17, 33, 3, mse=False, psnr=False, ssim=True)
    assert list(q.compute(a[:0].reshape(0, 33, 17, 3), a[:0].reshape(0, 33, 17, 3))) == []
    a = rng.integers(0, 256, (1, 33, 17, 3), dtype=np.uint8)
    assert list(q.compute(a, a)[0]) == ["ssim"]


def test_1080p_gray_and_4k_rgb():
    import torch
    A = _hip()
    rng = np.random.default_rng(4)
    for (W, H, Cn, n) in ((1920, 1080, 1, 4), (3840, 2160, 3, 1)):
        a = rng.integers(0, 256, (n, H, W, Cn), dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
        q = A.HipQuality(W, H, Cn, ssim=True)
        dmap = torch.empty(q.map_shape(n), dtype=torch.float64, device="cuda")
        got = q.compute_device(_cuda(a), _cuda(b), ssim_map=dmap)
        _check_frames(A, a, b, got, dmap.cpu().numpy())


def test_determinism_and_batch_independence():
    import torch
    A = _hip()
    rng = np.random.default_rng(6)
    W, H, T = 1920, 1080, 60
    base = rng.integers(0, 256, (H, W), dtype=np.uint8)
    d_a = torch.from_numpy(np.stack([np.roll(base, k, axis=1) for k in range(T)])[..., None]).cuda()
    noise = torch.from_numpy(rng.integers(-9, 10, (T, H, W, 1)).astype(np.int16)).cuda()
    d_b = (d_a.to(torch.int16) + noise).clamp(0, 255).to(torch.uint8)
    q = A.HipQuality(W, H, 1, ssim=True)
    s = torch.cuda.Stream()
    all1 = q.compute_device(d_a, d_b, stream=s)
    all2 = q.compute_device(d_a, d_b)
    key = lambda g: bits([g["mse"], g["psnr"], g["ssim"]]).tolist()
    assert [key(g) for g in all1] == [key(g) for g in all2]
    for k in (0, 17, 59):
        alone = q.compute_device(d_a[k:k + 1], d_b[k:k + 1])[0]
        host = q.compute(d_a[k].cpu().numpy(), d_b[k].cpu().numpy())[0]
        assert key(alone) == key(all1[k]) == key(host), k
    _check_frames(A, d_a[:1].cpu().numpy(), d_b[:1].cpu().numpy(), all1[:1])


def test_lossy_round_trip_framer_output_into_the_metrics():
    """1080p scene clip at the reference's default quality (crf 3: 2, 7, 7; Collapse, AbsoluteT, delta_t_max 7650):
    transcode and reframe on the device, and the framer's popped frames go into the device metrics on the same stream
    with no host synchronisation in between."""
    import torch
    A = _hip()
    W, H, T, dtm = 1920, 1080, 30, 7650
    base, cmax, vel = 2, 7, 7
    clip = O.synth_clip(O.CONTENT_SCENE, W, H, 1, T)
    kwf = dict(tps=255 * 30, ref_interval=255, delta_t_max=dtm, output_fps=30.0, codec_version=3,
               time_mode=A.TIME_ABSOLUTE_T)
    hv = A.HipVideo(W, H, 1, time_mode=A.TIME_ABSOLUTE_T, multi_mode=A.MULTI_COLLAPSE, delta_t_max=dtm,
                    c_thresh_start=base, c_counter_start=0, max_depth=20)
    hv.set_crf_parameters(cmax, vel)
    fr = A.HipFramer(W, H, 1, source_camera=A.FRAMED_U8, ring_frames=256, **kwf)
    q = A.HipQuality(W, H, 1, ssim=True)
    st = torch.cuda.current_stream().cuda_stream
    n_units = W * H
    d_clip = torch.from_numpy(clip.reshape(T, n_units)).cuda()
    got, recs = [], []
    popped = 0

    def drain(n):
        nonlocal popped, got
        d_out = torch.empty((n, n_units), dtype=torch.uint8, device="cuda")
        m = fr.pop_device(d_out, n, stream=st)
        if m:  # the popped frames straight into the metrics, same stream, no host wait in between
            got += q.compute_device(d_clip[popped:popped + m], d_out[:m], stream=st)
            recs.append(d_out[:m].cpu().numpy())
            popped += m
        return m

    for k0 in range(0, T, 10):
        d_ev = torch.empty((n_units * 10, 3), dtype=torch.int32, device="cuda")
        d_off = torch.zeros(11, dtype=torch.int64, device="cuda")
        hv.integrate_device(d_clip[k0:k0 + 10], d_ev, d_off, stream=st)
        hv.finish()
        fr.ingest_frames_device(d_ev, d_off.cpu().numpy().astype(np.uint64), stream=st)
        n = fr.frames_ready()
        if n:
            drain(n)
    # Collapse holds a frame back until its last pixel has spoken: the end-of-stream flush hands the rest out
    while popped < T and fr.flush_frame_buffer():
        assert drain(1) == 1
    assert popped >= 20
    rec = np.concatenate(recs).reshape(popped, H, W, 1)
    for i in range(popped):
        assert {"mse": got[i]["mse"], "psnr": got[i]["psnr"]} == A.calculate_quality_metrics(clip[i], rec[i]), i
    for i in range(0, popped, 4):
        s, _, _, abs_sums, _ = Q.fast_ssim(clip[i], rec[i], want_map=False)
        assert abs(got[i]["ssim"] - s) <= Q.ssim_bound(abs_sums, 1), i
    print(f"\n[quality] {popped} frames at crf 3: mean PSNR {np.mean([g['psnr'] for g in got]):.2f} dB, "
          f"mean SSIM {np.mean([g['ssim'] for g in got]):.4f}")


def test_viewer_loop_running_plane_on_one_stream():
    """The viewer's comparison (adder-viz transcoder/adder.rs:306-330): each input frame against the transcoder's
    running intensities, the plane copied on the device behind the 1-frame batch on the same stream."""
    import torch
    A = _hip()
    W, H, T = 64, 48, 12
    clip = O.synth_clip(O.CONTENT_SCENE, W, H, 1, T)
    ov = O.Video(W, H, 1, time_mode=O.ABSOLUTE_T, multi_mode=O.COLLAPSE, delta_t_max=7650)
    hv = A.HipVideo(W, H, 1, time_mode=A.TIME_ABSOLUTE_T, multi_mode=A.MULTI_COLLAPSE, delta_t_max=7650)
    hv.enable_running_intensities(True)
    for v in (ov, hv):
        v.set_crf_parameters(7, 7)
        v.reset_c_thresh(2)
    q = A.HipQuality(W, H, 1, ssim=True)
    s = torch.cuda.Stream()
    d_plane = torch.full((H, W, 1), 77, dtype=torch.uint8, device="cuda")
    d_clip = torch.from_numpy(clip.reshape(T, W * H)).cuda()
    torch.cuda.synchronize()
    for k in range(T):
        ov.integrate_matrix(clip[k])
        d_ev = torch.empty((hv.max_events_per_frame + 1024, 3), dtype=torch.int32, device="cuda")
        d_off = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        hv.integrate_device(d_clip[k:k + 1], d_ev, d_off, stream=s.cuda_stream)
        hv.running_intensities_device(d_plane, stream=s.cuda_stream)
        got = q.compute_device(d_clip[k].view(H, W, 1), d_plane, stream=s)[0]
        hv.finish()
        plane = d_plane.cpu().numpy()
        assert np.array_equal(plane, hv.running_intensities()), k
        assert np.array_equal(plane, ov.running_intensities().reshape(H, W, 1)), k
        assert {"mse": got["mse"], "psnr": got["psnr"]} == A.calculate_quality_metrics(clip[k], plane), k
        sref, _, _, abs_sums, _ = Q.fast_ssim(clip[k], plane, want_map=False)
        assert abs(got["ssim"] - sref) <= Q.ssim_bound(abs_sums, 1)


def test_running_plane_device_copy_before_enabling_is_zero():
    import torch
    A = _hip()
    hv = A.HipVideo(16, 8, 3)
    d = torch.full((8, 16, 3), 5, dtype=torch.uint8, device="cuda")
    hv.running_intensities_device(d)
    torch.cuda.synchronize()
    assert int(d.sum()) == 0


def test_errors_return_their_code_and_launch_nothing():
    import torch
    A = _hip()
    from adder_amd import quality
    N = A._native
    L = quality.load()
    h = C.c_void_p()
    for w, hh, ch, m, abi in ((0, 8, 1, 7, 1), (8, 0, 1, 7, 1), (8, 8, 2, 7, 1), (8, 8, 4, 7, 1), (8, 8, 1, 0, 1),
                              (8, 8, 1, 8, 1), (8, 8, 1, 7, 2)):
        p = quality.AdderQualityParams(abi_version=abi, width=w, height=hh, channels=ch, metrics=m)
        assert L.adder_quality_create(C.byref(p), C.byref(h)) == N.E_BAD_PARAMS
    assert L.adder_quality_create(None, C.byref(h)) == N.E_BAD_PARAMS
    q = A.HipQuality(16, 16, 1, ssim=False)
    d = torch.zeros((2, 16, 16, 1), dtype=torch.uint8, device="cuda")
    res = (quality.AdderQualityResult * 2)()
    res[0].mse = -1.0
    dmap = torch.full((2, 1, 9, 9), -3.0, dtype=torch.float64, device="cuda")
    for args in ((None, d.data_ptr(), 2, res, None), (d.data_ptr(), None, 2, res, None),
                 (d.data_ptr(), d.data_ptr(), 2, None, None),
                 (d.data_ptr(), d.data_ptr(), 2, res, dmap.data_ptr())):  # a map without SSIM in the mask
        assert L.adder_quality_compute_device(q.h, *args, None) == N.E_BAD_PARAMS
        assert L.adder_quality_last_error(q.h)
    assert L.adder_quality_compute_device(None, d.data_ptr(), d.data_ptr(), 2, res, None, None) == N.E_BAD_PARAMS
    torch.cuda.synchronize()
    assert res[0].mse == -1.0 and bool((dmap == -3.0).all())
    assert L.adder_hip_running_intensities_device(None, d.data_ptr(), None) == N.E_BAD_PARAMS
