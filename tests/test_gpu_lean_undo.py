"""The two-plane undo copy of batches that start with the packed frame kernel (adder_lp_kernel): the batch's first
launch keeps the header and delta_t planes it loads, an overflowing event buffer rolls the state back from those two
(adder_lp_restore_kernel: lr_pack of lr_unpack), and whatever follows -- the retry, the next batch, another kernel that
reads all four resident planes -- must see the state a run that never overflowed would.  DeltaT, Collapse, delta_t_max =
ref_time = 255, c_thresh 0 throughout (the packed kernel's regime); every comparison is byte for byte against the oracle,
through both outputs (AdderEvents and the raw sink's records), into guarded buffers (tests/test_gpu_packed_edges.py).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import clips
import test_gpu_packed_edges as E  # (its guarded buffers, oracle / context pairs and batch runner)

# three pairs of segments, the last one ragged (675 = 2 * 256 + 163 units): one workgroup; and eleven pairs (2751 units,
# the last ragged): three workgroups
SMALL = {1: (45, 15), 3: (15, 15)}
WIDE = {1: (131, 21), 3: (131, 7)}
PRE, NEXT = 7, 5  # frames in front of the batch that overflows (its planes are live), frames of the batch behind it


@functools.lru_cache(maxsize=None)
def _case(Cn, nb, wide=False):
    W, H = (WIDE if wide else SMALL)[Cn]
    clip = clips.make_clip("runs", PRE + nb + NEXT, H, W, Cn, seed=5 * nb + Cn)
    clip[PRE + nb // 2] = 0  # (intensity 0: black roots, the D_ZERO events)
    return clip, E._want(clip)


def _overflow(hv, form, clip, per, cap_bytes, tag):
    """Submits clip as ONE batch into a buffer of cap_bytes: E_OUT_CAPACITY with the size needed, the oracle's prefix in
    front of the capacity and not a byte behind it; the packed kernel ran."""
    import torch
    A = E._hip()
    Cn = clip.shape[3]
    rec = E._rec(form, Cn)
    n = sum(len(p) for p in per)
    cap = cap_bytes // rec
    assert cap < n, tag
    st = torch.cuda.current_stream().cuda_stream
    d_frames = torch.from_numpy(np.ascontiguousarray(clip).reshape(len(clip), -1)).cuda()
    buf = E._Guarded(n * rec)
    d_offs = torch.zeros(len(clip) + 1, dtype=torch.int64, device="cuda")
    E._submit(hv, form, d_frames, buf.out[:cap_bytes], d_offs, st)
    with pytest.raises(A.AdderHipError) as ei:
        hv.finish()
    assert hv.last_batch_kernel() == A.KERNEL_LEAN_RUNS_PACKED, tag
    assert ei.value.code == A.E_OUT_CAPACITY and hv.last_required == n, (tag, hv.last_required, n)
    buf.check(E._bytes(per, form, Cn), tag, written=cap * rec)


# ---- 1. capacities that end inside the stream, batches of one, two and three launches ------------------------------
@pytest.mark.parametrize("nb", [3, 60, 61, 130])
@pytest.mark.parametrize("Cn", [1, 3])
def test_rollback_at_every_capacity(Cn, nb):
    """Batches of 3, 60 (one launch), 61 (two) and 130 frames (three) behind a batch that left live planes: for every
    capacity the oracle's prefix, then the retry and the next batch as if nothing had happened."""
    for wide in (False, True) if nb in (3, 61) else (False,):
        clip, want = _case(Cn, nb, wide)
        W, H = (WIDE if wide else SMALL)[Cn]
        per = want[PRE:PRE + nb]
        n = sum(len(p) for p in per)
        assert n > len(per[0]) + 3 + 17
        for form in ("events", "wire"):
            rec = E._rec(form, Cn)
            caps = [0, (len(per[0]) + 3) * rec, (n - 17) * rec, (n - 1) * rec]
            if form == "wire":
                caps.append(n * rec - 1)
            hv = E._video(W, H, Cn)
            for cap_bytes in caps:
                tag = (Cn, nb, wide, form, cap_bytes)
                hv.reset()
                E._run(hv, clip[:PRE], want[:PRE], (PRE,), form, ("pre",) + tag)
                _overflow(hv, form, clip[PRE:PRE + nb], per, cap_bytes, tag)
                E._run(hv, clip[PRE:PRE + nb], per, (nb,), form, ("retry",) + tag)
                E._run(hv, clip[PRE + nb:], want[PRE + nb:], (NEXT,), form, ("next",) + tag)
            hv.close()


def test_rollback_twice_in_a_row_and_of_the_first_batch():
    """The stream's first batch (pristine planes: the level planes were never written) overflows twice with different
    capacities before it fits; so does the batch behind it."""
    clip, want = _case(1, 61)
    W, H = SMALL[1]
    for form in ("events", "wire"):
        rec = E._rec(form, 1)
        hv = E._video(W, H, 1)
        k = 0
        for nb in (PRE + 10, 51 + NEXT):
            per = want[k:k + nb]
            n = sum(len(p) for p in per)
            for cap in (n // 2, 0, n - 1):
                _overflow(hv, form, clip[k:k + nb], per, cap * rec, (form, k, cap))
            E._run(hv, clip[k:k + nb], per, (nb,), form, ("retry", form, k))
            k += nb
        assert k == len(clip)
        hv.close()


# ---- 2. the repack launch: another kernel reads all four resident planes behind the rollback -----------------------
def _pair(W, H, Cn, time_mode=O.DELTA_T):
    return E._oracle(W, H, Cn, time_mode=time_mode), E._video(W, H, Cn, time_mode=time_mode)


def _batch(ov, hv, frames, kernels, tag, overflow_by=None):
    """frames as one batch of integrate_batch against the oracle, the frame kernel asserted; overflow_by: a first attempt
    into a buffer that many events short."""
    A = E._hip()
    want = [ov.integrate_matrix(f) for f in frames]
    need = sum(len(w) for w in want)
    if overflow_by is not None:
        assert need > overflow_by
        with pytest.raises(A.AdderHipError) as ei:
            hv.integrate_batch(frames, out_cap=need - overflow_by)
        assert ei.value.code == A.E_OUT_CAPACITY and hv.last_required == need, tag
    got, offs = hv.integrate_batch(frames, out_cap=max(need, 1))
    assert hv.last_batch_kernel() in kernels, (tag, hv.last_batch_kernel())
    assert [int(offs[i + 1] - offs[i]) for i in range(len(frames))] == [len(w) for w in want], tag
    assert np.array_equal(got, np.concatenate(want)), tag


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("then", ["lean_crf", "lean", "lr", "one"])
def test_another_kernel_follows_the_rollback(monkeypatch, Cn, then):
    """A packed batch leaves live planes, the next packed batch (two launches) overflows and is rolled back, and the frames
    it held go through ANOTHER frame kernel: adder_lean_kernel at c_thresh > 0 (crf 3's parameters from here on) and at
    c_thresh 0, adder_lr_kernel, the one-frame kernel -- all of which read the integration and best-event planes the
    rollback rebuilt.  Then a packed batch again where the regime still allows it."""
    A = E._hip()
    W, H = WIDE[Cn]
    clip = clips.make_clip("runs", 20 + 61 + 30, H, W, Cn, seed=41 + Cn)
    clip[50] = 0
    ov, hv = _pair(W, H, Cn)
    _batch(ov, hv, clip[:20], {A.KERNEL_LEAN_RUNS_PACKED}, "pre")
    held = sum(len(ev) for ev in E._want(clip)[20:81])
    with pytest.raises(A.AdderHipError) as ei:
        hv.integrate_batch(clip[20:81], out_cap=held - 17)
    assert ei.value.code == A.E_OUT_CAPACITY and hv.last_required == held
    assert hv.last_batch_kernel() == A.KERNEL_LEAN_RUNS_PACKED
    if then == "lean_crf":
        for v in (ov, hv):
            v.set_crf_parameters(7, 7)
            v.reset_c_thresh(3)
        _batch(ov, hv, clip[20:81], {A.KERNEL_LEAN}, then)
        _batch(ov, hv, clip[81:], {A.KERNEL_LEAN}, then, overflow_by=5)
    elif then == "one":
        for k in range(20, 81):
            _batch(ov, hv, clip[k:k + 1], {A.KERNEL_LEAN}, (then, k))
        _batch(ov, hv, clip[81:], {A.KERNEL_LEAN_RUNS_PACKED}, then, overflow_by=5)
    else:
        monkeypatch.setenv("ADDER_HIP_NO_LR" if then == "lean" else "ADDER_HIP_NO_LP", "1")
        _batch(ov, hv, clip[20:81], {A.KERNEL_LEAN if then == "lean" else A.KERNEL_LEAN_RUNS}, then)
        monkeypatch.delenv("ADDER_HIP_NO_LR" if then == "lean" else "ADDER_HIP_NO_LP")
        _batch(ov, hv, clip[81:], {A.KERNEL_LEAN_RUNS_PACKED}, then, overflow_by=5)
    hv.close()


def test_absolute_t_follows_the_rollback_of_the_first_batch():
    """The time mode may change while no frame has been integrated -- a rolled-back first batch counts as none: the planes
    the rollback rebuilt from the pristine ones then go through adder_lr_kernel in AbsoluteT."""
    A = E._hip()
    W, H = WIDE[1]
    clip = clips.make_clip("runs", 70, H, W, 1, seed=53)
    hv = E._video(W, H, 1)
    held = sum(len(ev) for ev in E._want(clip[:61]))
    with pytest.raises(A.AdderHipError) as ei:
        hv.integrate_batch(clip[:61], out_cap=held - 17)
    assert ei.value.code == A.E_OUT_CAPACITY and hv.last_batch_kernel() == A.KERNEL_LEAN_RUNS_PACKED
    hv.set_time_mode(O.ABSOLUTE_T)
    ov = E._oracle(W, H, 1, time_mode=O.ABSOLUTE_T)
    _batch(ov, hv, clip[:61], {A.KERNEL_LEAN_RUNS}, "abs_t")
    _batch(ov, hv, clip[61:], {A.KERNEL_LEAN_RUNS}, "abs_t", overflow_by=3)
    hv.close()


# ---- 3. runs carried across the rolled-back batch -------------------------------------------------------------------
@pytest.mark.parametrize("W,Cn", [(256, 1), (86, 3)])
def test_escape_words_across_a_rollback(W, Cn):
    """tests/test_gpu_packed_edges.py's escape clip (runs of 250..261 frames end in frames 250..270) in batches of 64: the
    batches that hold the escaping records overflow first, so the runs they flush -- 192 and 256 frames old when the batch
    begins -- come out of the two-plane copy."""
    clip = E._escape_clip(W, Cn, staggered=True)
    lengths = np.concatenate([r for _, _, r in E._escape_runs(clip)])
    assert set(range(250, 262)) <= set(lengths.tolist())
    want = E._want(clip)
    for form in ("events", "wire"):
        rec = E._rec(form, Cn)
        hv = E._video(W, 3, Cn)
        k = 0
        for nb in (64, 64, 64, 64, 44):
            per = want[k:k + nb]
            n = sum(len(p) for p in per)
            if k >= 192:
                for cap in (n - 1, n // 3):
                    _overflow(hv, form, clip[k:k + nb], per, cap * rec, (W, Cn, form, k, cap))
            E._run(hv, clip[k:k + nb], per, (nb,), form, (W, Cn, form, k))
            k += nb
        hv.close()


def test_the_run_bound_survives_rollbacks():
    """The integer-state kernels run while rho * 255 stays below 2^24 for the longest run (65 793 frames), a bound the
    host keeps from the kernels' reports.  One static pixel: the packed kernel up to frame 65 536, the float kernel from
    there on -- with every batch around the switch rolled back first, the switch comes at the same batch.  No static
    pixel (every unit changes at least every 3 000 frames): rollbacks do not send the stream to the float kernel either."""
    A = E._hip()
    W, H, T, NB = 64, 1, 73728, 4096
    rng = np.random.default_rng(19)
    period = rng.integers(1000, 3000, (H, W, 1))
    phase = rng.integers(0, 3000, (H, W, 1))
    vals = rng.integers(0, 256, (64, H, W, 1)).astype(np.uint8)
    k = np.arange(T).reshape(T, 1, 1, 1)
    clip = np.take_along_axis(vals, ((k + phase[None]) // period[None]) % 64, axis=0)
    for one_static in (True, False):
        c = clip.copy()
        if one_static:
            c[:, 0, 37] = 131
        ov, hv = _pair(W, H, 1)
        kernels = []
        for b in range(T // NB):
            around = 13 <= b <= 17
            _batch(ov, hv, c[b * NB:(b + 1) * NB], {A.KERNEL_LEAN_RUNS_PACKED, A.KERNEL_LEAN}, (one_static, b),
                   overflow_by=1 if around else None)
            kernels.append(hv.last_batch_kernel())
        switch = 65536 // NB  # the first batch whose last frame would carry the static run past 65 793 frames
        if one_static:
            assert kernels == [A.KERNEL_LEAN_RUNS_PACKED] * switch + [A.KERNEL_LEAN] * (T // NB - switch), kernels
        else:
            assert kernels == [A.KERNEL_LEAN_RUNS_PACKED] * (T // NB), kernels
        hv.close()


# ---- 4. contexts that keep the whole-state copy ---------------------------------------------------------------------
def test_side_plane_keeps_the_whole_copy():
    """A context whose running-intensities plane exists keeps the copy of every plane (the plane is part of what a batch
    may change): one-frame batches while it is on, packed batches once it is off again -- rolled back like before."""
    A = E._hip()
    W, H = SMALL[1]
    clip = clips.make_clip("runs", 100, H, W, 1, seed=61)
    ov, hv = _pair(W, H, 1)
    hv.enable_running_intensities(True)
    _batch(ov, hv, clip[:6], {A.KERNEL_LEAN}, "side plane on", overflow_by=2)
    assert np.array_equal(hv.running_intensities(), ov.running_intensities())
    hv.enable_running_intensities(False)
    _batch(ov, hv, clip[6:70], {A.KERNEL_LEAN_RUNS_PACKED}, "side plane off", overflow_by=9)
    _batch(ov, hv, clip[70:], {A.KERNEL_LEAN_RUNS_PACKED}, "side plane off", overflow_by=1)
    hv.close()


def test_feature_context_keeps_the_whole_copy():
    """Feature-driven rate control (per-pixel c_thresh, the feature set, the side plane): never the packed kernel, the whole
    copy as before -- thresholds, feature set and side plane roll back with the pixels."""
    A = E._hip()
    W, H = 56, 40
    clip = clips.make_clip("corners", 20, H, W, 1, seed=13)
    ov = O.Video(W, H, 1, time_mode=O.DELTA_T, multi_mode=O.COLLAPSE, ref_time=255, delta_t_max=255)
    hv = A.HipVideo(W, H, 1, time_mode=O.DELTA_T, multi_mode=O.COLLAPSE, ref_time=255, delta_t_max=255, max_depth=24)
    ov.ensure_capacity(26)
    for v in (ov, hv):
        v.set_crf_parameters(7, 7)
        v.reset_c_thresh(2)
    ov.update_detect_features(True, True, 2, 5)
    hv.update_detect_features(True, True)
    hv.set_feature_parameters(2, 5)
    _batch(ov, hv, clip[:8], {A.KERNEL_GENERIC, A.KERNEL_BOUNDED, A.KERNEL_LEAN}, "features")
    assert hv.last_batch_kernel() != A.KERNEL_LEAN_RUNS_PACKED
    _batch(ov, hv, clip[8:], {A.KERNEL_GENERIC, A.KERNEL_BOUNDED, A.KERNEL_LEAN}, "features", overflow_by=40)
    assert np.array_equal(hv.c_thresh_plane(), ov.c_thresh_plane())
    assert np.array_equal(hv.feature_set(), ov.feature_set())
    hv.close()


# ---- 5. planes outside the regime -----------------------------------------------------------------------------------
def test_planes_outside_the_regime_never_reach_the_packed_kernel():
    """adder_lp_kernel checks the planes it loads (popped_dtm == (base_val != 0)) and reports a violation as an internal
    error (kStatusLeanRuns): the context is poisoned, nothing is rolled back -- only a pure capacity status is -- and the
    two-plane copy would hold the very planes that were refused.  No call sequence gets such planes in front of the packed
    kernel: here another kernel writes them (a window of two frames: a root of non-zero intensity is NOT popped in the frame
    it starts), the window then shrinks to the packed kernel's, and the batch plan keeps the generic step for good -- with
    the whole-state copy behind its rollback."""
    A = E._hip()
    W, H = SMALL[1]
    clip = clips.make_clip("runs", 40, H, W, 1, seed=71)
    ov = E._oracle(W, H, 1, dtm=510)
    hv = E._video(W, H, 1, dtm=510)
    others = {A.KERNEL_BOUNDED, A.KERNEL_CONSTANT_RUNS, A.KERNEL_RUN_RECORDS, A.KERNEL_GENERIC}
    _batch(ov, hv, clip[:8], others, "window of two")
    for v in (ov, hv):
        v.set_delta_t_max(255)
    _batch(ov, hv, clip[8:30], others, "window of one", overflow_by=7)
    _batch(ov, hv, clip[30:], others, "window of one", overflow_by=1)
    hv.close()
