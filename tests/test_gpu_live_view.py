"""The transcoder's live view on the GPU (include/adder_hip.h: adder_hip_set_view_mode, adder_hip_set_show_features,
adder_hip_display_frame[_device]) against the restatement on the CPU oracle (tests/live_view_oracle.py): the D, DeltaT
and SAE planes byte for byte after every frame and after a batch, events unchanged, detection reading the view plane,
the display frame with Instant / Hold crosses, sparse steps and row bands.

Planes are 70x37x1 and 33x19x3 (widths off every vector and wave multiple; more than one segment), clips 24 frames of
scene content with one quarter static and one quarter noise.  A restatement run is shared by the cases that use it."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
import live_view_oracle as R

pytestmark = pytest.mark.gpu

T = 24
PLANES = [(70, 37, 1), (33, 19, 3)]
VIEWS = [R.VIEW_INTENSITY, R.VIEW_D, R.VIEW_DELTA_T, R.VIEW_SAE]
MAX_DEPTH = 30


def _hip():
    import adder_amd
    return adder_amd


@functools.lru_cache(maxsize=None)
def _clip(W, H, Cn):
    c = R.live_clip(W, H, Cn, T)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _trace(W, H, Cn, time_mode, dtm, pixel_mode):
    """The clip through the restatement once: per frame the events and the plane in every view."""
    lv = R.LiveView(W, H, Cn, time_mode=time_mode, delta_t_max=dtm, pixel_mode=pixel_mode)
    frames = []
    for k in range(T):
        ev = lv.step(_clip(W, H, Cn)[k])
        frames.append((ev, {v: p.copy() for v, p in lv.planes.items()}))
    return frames, lv.collapsed_pops


def _video(A, W, H, Cn, time_mode, dtm, pixel_mode=0, view=None, **kw):
    hv = A.HipVideo(W, H, Cn, time_mode=time_mode, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=dtm,
                    max_depth=MAX_DEPTH, pixel_mode=pixel_mode, **kw)
    hv.enable_running_intensities(True)
    if view is not None:
        hv.set_view_mode(view)
    return hv


# ---- 1. views x kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", VIEWS, ids=["intensity", "d", "delta_t", "sae"])
@pytest.mark.parametrize("dtm", [255, 510, 7650])
@pytest.mark.parametrize("time_mode", [O.DELTA_T, O.ABSOLUTE_T], ids=["delta_t", "absolute_t"])
@pytest.mark.parametrize("W,H,Cn", PLANES)
def test_views_frame_perfect(W, H, Cn, time_mode, dtm, view):
    """dtm 255: the lean regime (the Intensity control runs the lean kernel, the views the generic one); 510 = 2 ref_time:
    the static quarter takes the Collapse pop of a popped arena (event_pixel_tree.rs:257), what SAE in DeltaT rests on;
    7650: deep arenas."""
    A = _hip()
    frames, collapsed = _trace(W, H, Cn, time_mode, dtm, O.FRAME_PERFECT)
    if dtm == 510:
        assert collapsed > 0
    assert any(not np.array_equal(frames[-1][1][view], frames[-1][1][v]) for v in VIEWS if v != view)
    clip = _clip(W, H, Cn)
    hv = _video(A, W, H, Cn, time_mode, dtm, view=view)
    for k in range(T):
        got = hv.integrate_matrix(clip[k])
        kernel = hv.last_batch_kernel()
        if view != R.VIEW_INTENSITY:
            assert kernel == A.KERNEL_GENERIC, (k, A.KERNEL_NAMES[kernel])
        else:   # the control runs what it ran before the views existed
            assert kernel == (A.KERNEL_LEAN if dtm == 255 else A.KERNEL_BOUNDED), (k, A.KERNEL_NAMES[kernel])
        assert np.array_equal(got, frames[k][0]), k
        assert np.array_equal(hv.running_intensities(), frames[k][1][view]), k
    hv.close()
    hb = _video(A, W, H, Cn, time_mode, dtm, view=view)
    got, offs = hb.integrate_batch(clip, out_cap=hb.max_events_per_frame * T)
    assert np.array_equal(got, np.concatenate([f[0] for f in frames]))
    assert np.array_equal(hb.running_intensities(), frames[-1][1][view])
    if view != R.VIEW_INTENSITY:
        assert hb.last_batch_kernel() == A.KERNEL_GENERIC
    hb.close()


@pytest.mark.parametrize("view", VIEWS, ids=["intensity", "d", "delta_t", "sae"])
@pytest.mark.parametrize("dtm", [510, 7650])
@pytest.mark.parametrize("time_mode", [O.DELTA_T, O.ABSOLUTE_T], ids=["delta_t", "absolute_t"])
def test_views_continuous_kernel(time_mode, dtm, view):
    A = _hip()
    W, H, Cn = PLANES[1]
    frames, _ = _trace(W, H, Cn, time_mode, dtm, O.CONTINUOUS)
    clip = _clip(W, H, Cn)
    hv = _video(A, W, H, Cn, time_mode, dtm, pixel_mode=1, view=view)
    for k in range(T):
        got = hv.integrate_matrix(clip[k])
        assert hv.last_batch_kernel() == A.KERNEL_CONTINUOUS
        assert np.array_equal(got, frames[k][0]), k
        assert np.array_equal(hv.running_intensities(), frames[k][1][view]), k
    hv.close()
    hb = _video(A, W, H, Cn, time_mode, dtm, pixel_mode=1, view=view)
    got, _ = hb.integrate_batch(clip, out_cap=hb.max_events_per_frame * T)
    assert np.array_equal(got, np.concatenate([f[0] for f in frames]))
    assert np.array_equal(hb.running_intensities(), frames[-1][1][view])
    hb.close()


def test_bad_arguments():
    A = _hip()
    hv = A.HipVideo(16, 8, 1)
    for call in (lambda: hv.set_view_mode(4), lambda: hv.set_show_features(3), lambda: hv.set_view_mode(1, float("nan")),
                 lambda: hv.display_frame()):   # (the plane was never enabled)
        with pytest.raises(A.AdderHipError) as e:
            call()
        assert e.value.code == A.E_BAD_PARAMS
    hv.close()


# ---- 2. set_delta_t_max mid-stream ------------------------------------------------------------------------------------
@pytest.mark.parametrize("time_mode", [O.DELTA_T, O.ABSOLUTE_T], ids=["delta_t", "absolute_t"])
def test_set_delta_t_max_mid_stream(time_mode):
    """The DeltaT / SAE denominators and the default practical_d_max follow from the next frame on; a pinned
    practical_d_max stays."""
    A = _hip()
    W, H, Cn = PLANES[1]
    clip = _clip(W, H, Cn)
    lv = R.LiveView(W, H, Cn, time_mode=time_mode, delta_t_max=7650)
    pinned = R.LiveView(W, H, Cn, time_mode=time_mode, delta_t_max=7650, view=R.VIEW_D, practical_d_max=32.0)
    hvs = {v: _video(A, W, H, Cn, time_mode, 7650, view=v) for v in VIEWS[1:]}
    hp = _video(A, W, H, Cn, time_mode, 7650)
    hp.set_view_mode(R.VIEW_D, 32.0)
    assert R.practical_d_max_exact(7650, 255) != R.practical_d_max_exact(2550, 255)
    for k in range(T):
        if k == 9:
            for x in [lv, pinned, hp] + list(hvs.values()):
                x.set_delta_t_max(2550)
        ev = lv.step(clip[k])
        pinned.step(clip[k])
        for v, hv in hvs.items():
            assert np.array_equal(hv.integrate_matrix(clip[k]), ev), (k, v)
            assert np.array_equal(hv.running_intensities(), lv.planes[v]), (k, v)
        hp.integrate_matrix(clip[k])
        assert np.array_equal(hp.running_intensities(), pinned.plane), k
    for hv in list(hvs.values()) + [hp]:
        hv.close()


# ---- 3. a view switch mid-stream --------------------------------------------------------------------------------------
@pytest.mark.parametrize("time_mode", [O.DELTA_T, O.ABSOLUTE_T], ids=["delta_t", "absolute_t"])
def test_view_switch_mid_stream(time_mode):
    """Intensity -> D -> SAE -> Intensity: a unit without a best event keeps the byte of the view it was last written in.
    With delta_t_max = 2 ref_time a root that fired in two frames running is popped at the second (pop_top_event,
    event_pixel_tree.rs:139-210) and leaves the pristine tail as root: no best event until the next frame.  After frame 1
    that is every unit of non-zero intensity, so the switch at frame 1 leaves frame 0's Intensity bytes standing under D;
    later it is the units that changed the frame before and kept still in this one.  (A unit that goes black is no such
    unit: 0 >= D_SHIFT[128] = 0 fires it at d = 128, which is 0 in Intensity and saturates D -- the block below.)"""
    A = _hip()
    W, H, Cn = PLANES[0]
    clip = _clip(W, H, Cn).copy()
    clip[:, 20:26, 40:52] = np.maximum(clip[:, 20:26, 40:52], 40)
    clip[5:, 20:26, 40:52] = 0
    lv = R.LiveView(W, H, Cn, time_mode=time_mode, delta_t_max=510)
    hv = _video(A, W, H, Cn, time_mode, 510)
    schedule = {1: R.VIEW_D, 12: R.VIEW_SAE, 18: R.VIEW_INTENSITY}
    for k in range(T):
        if k in schedule:
            before = lv.plane.copy()
            lv.set_view(schedule[k])
            hv.set_view_mode(schedule[k])
        assert np.array_equal(hv.integrate_matrix(clip[k]), lv.step(clip[k])), k
        if k in schedule:   # on the restatement alone: units without a best event exist and hold their old, non-zero byte
            nb = lv.no_best.reshape(lv.plane.shape)
            assert nb.any() and (lv.plane[nb] == before[nb]).all() and (lv.plane[nb] != 0).any(), k
            assert (lv.plane[~nb] != before[~nb]).any(), k   # ... while written units show the new view
        if k == 1:
            assert nb[: H // 2, : W // 2].sum() > H * W // 8   # (the static quarter, but for its black pixels)
        if k == 5:   # the block that went black: d = 128
            assert (lv.plane[20:26, 40:52] == 255).all()
        assert np.array_equal(hv.running_intensities(), lv.plane), k
    hv.close()


# ---- 4. detection reads the view plane --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _feature_run(view):
    W, H, Cn = PLANES[0]
    lv = R.LiveView(W, H, Cn, time_mode=O.ABSOLUTE_T, delta_t_max=7650, view=view, detect=True, adjust=True,
                    c_thresh_baseline=2, feature_c_radius=2)
    lv.reset_c_thresh(2)
    out = []
    for k in range(T):
        ev = lv.step(_clip(W, H, Cn)[k])
        out.append((ev, lv.plane.copy(), lv.feature_set.copy(), len(lv.new_features), lv.c_thresh_plane()))
    return out


@pytest.mark.parametrize("view", [R.VIEW_D, R.VIEW_SAE], ids=["d", "sae"])
def test_detection_in_a_view(view):
    A = _hip()
    W, H, Cn = PLANES[0]
    want, control = _feature_run(view), _feature_run(R.VIEW_INTENSITY)
    assert want[-1][2].any() and not np.array_equal(want[-1][2], control[-1][2])       # other features than Intensity's
    assert not np.array_equal(want[-1][4], control[-1][4])                             # ... and other low c_thresh squares
    hv = _video(A, W, H, Cn, O.ABSOLUTE_T, 7650, view=view)
    hv.set_crf_parameters(7, 7)
    hv.reset_c_thresh(2)
    hv.update_detect_features(True, True)
    hv.set_feature_parameters(2, 2)
    for k in range(T):
        ev, plane, fset, n_new, cth = want[k]
        assert np.array_equal(hv.integrate_matrix(_clip(W, H, Cn)[k]), ev), k
        assert hv.last_new_features() == n_new, k
        assert np.array_equal(hv.running_intensities(), plane), k
        assert np.array_equal(hv.feature_set(), fset), k
        assert np.array_equal(hv.c_thresh_plane(), cth), k
    hv.close()


# ---- 5. the display frame ---------------------------------------------------------------------------------------------
def _corner_clip(W, H, Cn):
    """Isolated bright pixels on black (FAST corners by construction): the four placements nearest the border, a pair 2
    apart in x and a pair 3 apart in y, switched on in different frames."""
    on = {(3, 3): 0, (W - 4, 3): 0, (3, H - 4): 1, (W - 4, H - 4): 1, (12, 9): 0, (14, 9): 2, (20, 8): 1, (20, 11): 3}
    clip = np.zeros((7, H, W, Cn), np.uint8)
    for (x, y), k0 in on.items():
        for k in range(k0, len(clip)):
            clip[k, y, x] = 255 if k % 2 == 0 else 200   # (beyond c_thresh every frame: the pixel pops, and is looked at)
    return clip


@pytest.mark.parametrize("show", [R.SHOW_OFF, R.SHOW_INSTANT, R.SHOW_HOLD], ids=["off", "instant", "hold"])
@pytest.mark.parametrize("W,H,Cn", PLANES)
def test_display_frame(W, H, Cn, show):
    import torch
    A = _hip()
    clip = _corner_clip(W, H, Cn)
    # (one row chunk: the circular event windows pair every lit pixel with another one, video.rs:901-903)
    lv = R.LiveView(W, H, Cn, time_mode=O.ABSOLUTE_T, delta_t_max=7650, detect=True, show=show, chunk_rows=H)
    hv = _video(A, W, H, Cn, O.ABSOLUTE_T, 7650, chunk_rows=H)
    hv.update_detect_features(True, False)
    hv.set_show_features(show)
    n = W * H * Cn
    differ = 0
    for k in range(len(clip)):
        assert np.array_equal(hv.integrate_matrix(clip[k]), lv.step(clip[k])), k
        assert np.array_equal(hv.feature_set(), lv.feature_set), k
        assert np.array_equal(hv.display_frame(), lv.display), k
        for off in (1, 4, 15):
            buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
            hv.display_frame_device(buf[off:off + n], stream=torch.cuda.current_stream().cuda_stream)
            got = buf.cpu().numpy()
            assert (got[:off] == 0xA5).all() and (got[off + n:] == 0xA5).all(), (k, off)
            assert np.array_equal(got[off:off + n].reshape(H, W, Cn), lv.display), (k, off)
        differ += not np.array_equal(lv.display, R.draw_crosses(lv.plane, [(x, y) for y, x in zip(*np.nonzero(lv.feature_set))]))
    fs = lv.feature_set
    assert fs[:, 3].any() and fs[:, W - 4].any() and fs[3, :].any() and fs[H - 4, :].any()   # crosses reach every border zone
    assert fs[9, 12] and fs[9, 14] and fs[8, 20] and fs[11, 20]                              # two pairs of overlapping crosses
    if show == R.SHOW_HOLD:
        assert differ == 0 and (lv.display != lv.plane).any()
    else:
        assert differ > 0   # Off and Instant differ from Hold in some frame
    if show == R.SHOW_OFF:
        assert np.array_equal(lv.display, lv.plane)
    # detection off: the frame is the plane, whatever the mode
    hv.update_detect_features(False, False)
    hv.integrate_matrix(clip[-1])
    assert np.array_equal(hv.display_frame(), hv.running_intensities())
    hv.close()


# ---- 6. sparse steps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", VIEWS[1:], ids=["d", "delta_t", "sae"])
@pytest.mark.parametrize("time_mode", [O.DELTA_T, O.ABSOLUTE_T], ids=["delta_t", "absolute_t"])
def test_sparse_steps(time_mode, view):
    A = _hip()
    W, H = 21, 13
    rng = np.random.default_rng(5)
    lv = R.LiveView(W, H, 1, time_mode=time_mode, delta_t_max=40, ref_time=20, pixel_mode=O.CONTINUOUS, view=view)
    hv = A.HipVideo(W, H, 1, time_mode=time_mode, multi_mode=A.MULTI_COLLAPSE, ref_time=20, delta_t_max=40, max_depth=24,
                    pixel_mode=1)
    hv.enable_running_intensities(True)
    hv.set_view_mode(view)
    seen = 0
    for call in range(3):
        st = np.zeros(300, A.SPARSE_STEP_DTYPE)
        st["x"], st["y"], st["c"] = rng.integers(0, W, 300), rng.integers(0, H, 300), 0xFF
        st["x"][:40], st["y"][:40] = 5, 6            # a hot pixel: repeats inside the call
        st["frame_val"] = rng.choice([0, 3, 90, 200, 255], 300)
        st["intensity"] = st["frame_val"]
        st["time"] = rng.choice([1.0, 7.0, 20.0, 33.0], 300)
        want = lv.step_sparse(st)
        got = hv.integrate_sparse(st)
        assert np.array_equal(got, want), call
        assert np.array_equal(hv.running_intensities(), lv.plane), call
        seen += len(want)
    assert seen > 100 and lv.plane.any()
    if time_mode == O.DELTA_T:
        assert lv.collapsed_pops > 0
    hv.close()


# ---- 7. row bands -----------------------------------------------------------------------------------------------------
def test_row_bands():
    A = _hip()
    W, H, Cn = PLANES[0]
    clip = _clip(W, H, Cn)
    frames, _ = _trace(W, H, Cn, O.ABSOLUTE_T, 7650, O.FRAME_PERFECT)
    whole = _video(A, W, H, Cn, O.ABSOLUTE_T, 7650, view=R.VIEW_D)
    bands = [_video(A, W, H, Cn, O.ABSOLUTE_T, 7650, view=R.VIEW_D, row_begin=a, row_end=b) for a, b in ((0, 19), (19, 37))]
    for k in range(8):
        whole.integrate_matrix(clip[k])
        for hv in bands:
            hv.integrate_matrix(clip[k, hv.row_begin:hv.row_end])
            assert np.array_equal(hv.running_intensities(), whole.running_intensities()[hv.row_begin:hv.row_end]), k
    assert np.array_equal(whole.running_intensities(), frames[7][1][R.VIEW_D])
    for hv in bands:
        for call in (lambda: hv.set_show_features(R.SHOW_HOLD), hv.display_frame):
            with pytest.raises(A.AdderHipError) as e:
                call()
            assert e.value.code == A.E_BAD_PARAMS
        hv.set_show_features(R.SHOW_OFF)
        hv.close()
    whole.close()


# ---- 8. the C++ mirror ------------------------------------------------------------------------------------------------
def test_mirror_sae_view_with_held_features():
    """Video::instantaneous_view_mode(SAE) + ShowFeatureMode::Hold over 12 frames of 70x37: display_frame_features()."""
    import live_view_host_py as M
    W, H, Cn = PLANES[0]
    clip = _clip(W, H, Cn)[:12]
    lv = R.LiveView(W, H, Cn, time_mode=O.ABSOLUTE_T, delta_t_max=7650, c_thresh_max=7, c_increase_velocity=7, view=R.VIEW_SAE,
                    detect=True, show=R.SHOW_HOLD)
    n = 0
    for f in clip:
        n += len(lv.step(f))
    assert lv.feature_set.any() and (lv.display != lv.plane).any()
    got_n, running, display = M.live_view(clip, view=R.VIEW_SAE, detect=True, show=R.SHOW_HOLD)
    assert got_n == n
    assert np.array_equal(running, lv.plane)
    assert np.array_equal(display, lv.display)
    # the D view with a pinned divisor, no detection: the frame is the plane
    lv = R.LiveView(W, H, Cn, time_mode=O.ABSOLUTE_T, delta_t_max=7650, view=R.VIEW_D, practical_d_max=32.0)
    for f in clip:
        lv.step(f)
    _, running, display = M.live_view(clip, view=R.VIEW_D, practical_d_max=32.0)
    assert np.array_equal(running, lv.plane) and np.array_equal(display, lv.plane)
