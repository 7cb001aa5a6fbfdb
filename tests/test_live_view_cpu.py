"""The live view on the CPU: the restatement (tests/live_view_oracle.py) against oracle.Video in the Intensity view, the
shared value function and the cross decision (adder_pixel.hpp, built by g++) against the restatement, the batch plan's
side_view input, and the C-ABI / mirror exports."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import live_view_oracle as R
import live_view_sim_py as S
from oracle import oracle as O

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_the_oracle_in_the_intensity_view():
    """48x40 gray, 30 frames, feature_rate_adjustment on: running_intensities, feature_set, new_features and
    c_thresh_plane frame by frame, and the events."""
    W, H, T = 48, 40, 30
    clip = R.live_clip(W, H, 1, T)
    radius = 3
    ov = O.Video(W, H, 1, time_mode=O.ABSOLUTE_T, multi_mode=O.COLLAPSE, ref_time=255, delta_t_max=7650)
    ov.set_crf_parameters(7, 7)
    ov.reset_c_thresh(2)
    ov.update_detect_features(True, True, 2, radius)
    lv = R.LiveView(W, H, 1, time_mode=O.ABSOLUTE_T, delta_t_max=7650, c_thresh_max=7, c_increase_velocity=7, detect=True,
                    adjust=True, c_thresh_baseline=2, feature_c_radius=radius)
    lv.reset_c_thresh(2)
    seen_new = 0
    for k in range(T):
        want = ov.integrate_matrix(clip[k])
        got = lv.step(clip[k])
        assert np.array_equal(got, want), k
        assert np.array_equal(lv.plane, ov.running_intensities()), k
        assert np.array_equal(lv.feature_set, ov.feature_set()), k
        assert sorted(x | (y << 16) for x, y in lv.new_features) == sorted(ov.new_features().tolist()), k
        assert np.array_equal(lv.c_thresh_plane(), ov.c_thresh_plane()), k
        seen_new += len(lv.new_features)
    assert lv.check_c_thresh_against_pixels()
    assert seen_new > 0 and lv.feature_set.any()   # (the clip exercises what it compares)


D_ALL = np.arange(256, dtype=np.uint32)
T_GRID = np.array([0, 1, 254, 255, 256, 7649, 7650, 7651, 1 << 24, (1 << 32) - 1], np.uint32)
DTM_GRID = [0, 1, 255, 510, 7650, (1 << 32) - 1]
PDM_GRID = [0.0, 1.0, 7.99, 12.0, 32.0]


def test_value_function_intensity_and_d():
    d, t = np.meshgrid(D_ALL, T_GRID, indexing="ij")
    for ref in (255, 510, 1):
        want = R.view_value(R.VIEW_INTENSITY, d, t, 0, 0, ref, 7650, 1.0).reshape(-1)
        assert np.array_equal(S.values(R.VIEW_INTENSITY, ref, 7650, 1.0, d, t, 0, 0), want), ref
    for pdm in PDM_GRID:
        want = R.view_value(R.VIEW_D, d, t, 0, 0, 255, 7650, pdm).reshape(-1)
        assert np.array_equal(S.values(R.VIEW_D, 255, 7650, pdm, d, t, 0, 0), want), pdm
    # (the grid is not degenerate)
    assert len(np.unique(R.view_value(R.VIEW_D, D_ALL, 0, 0, 0, 255, 7650, 12.0))) == 13   # d = 0 .. 12 differ, then 255


def test_value_function_delta_t_and_sae():
    for dtm in DTM_GRID:
        want = R.view_value(R.VIEW_DELTA_T, 7, T_GRID, 0, 0, 255, dtm, 1.0).reshape(-1)
        assert np.array_equal(S.values(R.VIEW_DELTA_T, 255, dtm, 1.0, 7, T_GRID, 0, 0), want), dtm
        # SAE: every pair of the time grid, both orders -- last_fired > running wraps
        run, last = np.meshgrid(T_GRID, T_GRID, indexing="ij")
        want = R.view_value(R.VIEW_SAE, 7, 0, run, last, 255, dtm, 1.0).reshape(-1)
        assert np.array_equal(S.values(R.VIEW_SAE, 255, dtm, 1.0, 7, 0, run, last), want), dtm
    assert (np.meshgrid(T_GRID, T_GRID, indexing="ij")[1] > np.meshgrid(T_GRID, T_GRID, indexing="ij")[0]).any()
    # known answers: a wrapped difference of 2^32 - 254 ticks saturates; 255 of 510 ticks is half scale
    assert S.values(R.VIEW_SAE, 255, 510, 1.0, 0, 0, 1, 255)[0] == 255
    assert S.values(R.VIEW_SAE, 255, 510, 1.0, 0, 0, 510, 255)[0] == 127
    assert S.values(R.VIEW_DELTA_T, 255, 510, 1.0, 0, 255, 0, 0)[0] == 127
    assert S.values(R.VIEW_D, 255, 510, 8.0, 4, 0, 0, 0)[0] == 127


@pytest.mark.parametrize("w,h", [(7, 7), (16, 9), (33, 19), (70, 37)])
@pytest.mark.parametrize("ch", [1, 3])
def test_cross_decision_against_the_literal_scatter(w, h, ch):
    rng = np.random.default_rng(w * 100 + h + ch)
    plane = rng.integers(0, 255, (h, w, ch), dtype=np.uint8)   # (254 at most: a 255 is a cross)
    for density in (0.0, 0.02, 0.2):
        m = (rng.random((h, w)) < density).astype(np.uint8)
        if density:
            # members closer than 3 to every border, corners included: the restatement clips, the gather clamps
            for x, y in [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (1, h // 2), (w - 2, h // 2), (w // 2, 1), (w // 2, h - 2)]:
                m[y, x] = 1
        ys, xs = np.nonzero(m)
        want = R.draw_crosses(plane, list(zip(xs.tolist(), ys.tolist())))
        assert np.array_equal(S.display(plane, m), want), (w, h, ch, density)
        if density:
            assert (want != plane).any()


# ---- the batch plan's side_view input -------------------------------------------------------------------------------
import test_batch_plan as P  # noqa: E402  (its library, constants and regime table)


class PlanIn2(C.Structure):
    """BatchPlanIn with the side_view byte that sits behind wire_batch (tests/test_batch_plan.py's struct without it has
    the same size and offsets: the byte was padding)."""
    _fields_ = P.PlanIn._fields_[:P.PlanIn._fields_.index(("wire_batch", C.c_uint8)) + 1] + [("side_view", C.c_uint8)] + \
        P.PlanIn._fields_[P.PlanIn._fields_.index(("wire_batch", C.c_uint8)) + 1:]


VIEW_BIT = 16384
SERVES_VIEWS = {"GENERIC", "CONTINUOUS"}   # the frame kernels with a view instantiation (adder_launch_frame)


def _plan2(**kw):
    i = PlanIn2(**{**P.BASE, **kw})
    p = P.Plan()
    P.lib().plan_batch_c(C.cast(C.byref(i), C.POINTER(P.PlanIn)), C.byref(p))
    return p


def test_plan_struct_keeps_its_layout():
    assert C.sizeof(PlanIn2) == C.sizeof(P.PlanIn) == P.lib().plan_in_size()
    for name, _ in P.PlanIn._fields_:
        assert getattr(PlanIn2, name).offset == getattr(P.PlanIn, name).offset, name


@pytest.mark.parametrize("name,kw,want,bits_set,bits_clear", P.CASES, ids=[c[0] for c in P.CASES])
def test_plan_views_choose_only_kernels_that_serve_them(name, kw, want, bits_set, bits_clear):
    names = {v: k for k, v in P.K.items()}
    for time_mode, view in itertools.product((P.DELTA_T, P.ABSOLUTE_T), (0, 1, 2, 3)):
        over = dict(kw, time_mode=kw.get("time_mode", time_mode), launch_depth=1, side_view=view)  # (plane on: depth 1)
        p = _plan2(**over)
        k = names[P.kernel(p)]
        if view == 0:
            assert not p.variant & VIEW_BIT
            q = P.plan(**{k_: v for k_, v in over.items() if k_ != "side_view"})
            assert (p.variant, p.scratch, p.lean) == (q.variant, q.scratch, q.lean), name   # the Intensity view: as before
        elif p.refused is None:
            assert k in SERVES_VIEWS and p.variant & VIEW_BIT, (name, view, k)
            assert not p.variant & (P.BOUNDED | P.CONST_RUNS | P.RUN_RECORDS | P.LEAN_RUNS | P.PACKED), (name, p.variant)
            assert p.generic_sticky == (0 if kw.get("continuous") else 1)
            assert p.scratch in ((P.SCRATCH_NONE,) if kw.get("continuous") else (P.SCRATCH_LOG2, P.SCRATCH_LOG3))
        else:
            assert kw.get("records_only") or kw.get("wire_batch"), name   # (records need the lean regime: refused, not run)
    wc = P.lib().plan_worst_case_events_per_frame
    i = PlanIn2(**{**P.BASE, **kw, "side_view": 3})
    if not kw.get("continuous"):
        assert wc(C.cast(C.byref(i), C.POINTER(P.PlanIn))) == (P.BASE["max_depth"] + 1) * i.n_units   # a generic batch's bound


# ---- exports ----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("adder_hip_set_view_mode", "adder_hip_set_show_features", "adder_hip_display_frame", "adder_hip_display_frame_device")


def test_header_and_loader_name_the_new_entry_points():
    import adder_amd._native as N
    hdr = open(os.path.join(_ROOT, "include", "adder_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, hdr) and s in N.SYMBOLS, s
    lib_path = N.LIB_PATH
    assert os.path.exists(lib_path), "libadder_hip.so is not built"
    L = C.CDLL(lib_path)
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
    # argument checks need no device: a null context is ADDER_E_BAD_PARAMS
    assert L.adder_hip_set_view_mode(None, 0, C.c_float(0.0)) == N.E_BAD_PARAMS
    assert L.adder_hip_set_show_features(None, 0) == N.E_BAD_PARAMS
    assert L.adder_hip_display_frame(None, None) == N.E_BAD_PARAMS
    assert L.adder_hip_display_frame_device(None, None, None) == N.E_BAD_PARAMS


def test_practical_d_max_exact():
    import adder_amd as A
    assert A.practical_d_max_exact(7650, 255) == float(R.practical_d_max_exact(7650, 255)) == float(np.float32(np.log2(7650.0)))
    assert A.practical_d_max_exact(510, 255) == float(np.float32(np.log2(510.0)))
    assert A.practical_d_max_exact(7650, 510) == float(np.float32(np.log2(255.0 * 15)))   # (integer division)


def test_mirror_exports_the_live_view_helper():
    lib_path = os.path.join(_ROOT, "adder-codec-rs_amd", "host", "libadder_host.so")
    assert os.path.exists(lib_path), "libadder_host.so is not built"
    import subprocess
    names = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    assert " adder_host_live_view" in names
