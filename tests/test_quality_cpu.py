"""Quality metrics (include/adder_quality.h) without a GPU: known answers of the literal restatement of cv.rs:306-430
(tests/quality_oracle.py), the vectorised integer-moment form against it bit for bit, the library's symbol table and
its refusal to run without a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import kernel_constants
import quality_edge_cases as E
import quality_oracle as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


# ---- known answers of the literal form -----------------------------------------------------------------------

def test_constants_print_as_the_reference_evaluates_them():
    assert repr(Q.C1) == "6.502500000000001"
    assert repr(Q.C2) == "58.522499999999994"


def test_identical_frames():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (11, 13, 3), dtype=np.uint8)
    ssim, m, scores = Q.literal_ssim(a, a)
    assert ssim == 100.0 and (m == 1.0).all() and scores == [1.0, 1.0, 1.0]
    mse, psnr = Q.mse_psnr(a, a)
    assert mse == 1e-7 and psnr == 20.0 * math.log10(255.0) + 70.0


def test_constant_frames_closed_form():
    for x, y in ((0, 0), (10, 200), (255, 0), (77, 78)):
        a = np.full((9, 10), x, np.uint8)
        b = np.full((9, 10), y, np.uint8)
        _, m, _ = Q.literal_ssim(a, b)
        want = ((2.0 * x * y + Q.C1) * Q.C2) / ((float(x * x) + float(y * y) + Q.C1) * Q.C2)
        assert m.shape == (1, 2, 3) and (m == want).all(), (x, y, m[0, 0, 0], want)


def test_inverted_frame_is_negative():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    ssim, _, _ = Q.literal_ssim(a, 255 - a)
    assert -100.0 < ssim < -90.0


def test_a_plane_below_eight_rows_has_no_window():
    a = np.zeros((7, 20), np.uint8)
    ssim, m, _ = Q.literal_ssim(a, a + 1)
    assert math.isnan(ssim) and m.size == 0
    assert math.isnan(Q.fast_ssim(a, a + 1)[0])
    assert Q.mse_psnr(a, a + 1)[0] == 1.0


# ---- the vectorised form equals the literal one bit for bit --------------------------------------------------

def _pairs(rng, shape):
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    near = np.clip(a.astype(np.int16) + rng.integers(-3, 4, shape), 0, 255).astype(np.uint8)
    yield a, near
    yield a, rng.integers(0, 256, shape, dtype=np.uint8)
    yield a, 255 - a
    yield a, a


@pytest.mark.parametrize("shape", [(8, 8), (9, 13), (17, 11, 3), (23, 37), (16, 16, 3), (8, 30, 3), (12, 8)])
def test_fast_form_equals_the_literal_one(shape):
    rng = np.random.default_rng(sum(shape) * 7919)
    for a, b in _pairs(rng, shape):
        ls, lm, lsc = Q.literal_ssim(a, b)
        fs, fm, fsc, _, _ = Q.fast_ssim(a, b)
        assert (bits(lm) == bits(fm)).all(), shape
        assert bits(lsc).tolist() == bits(fsc).tolist()
        assert bits(ls) == bits(fs)


def test_fast_form_sequential_sum_is_cumsum():
    t = np.array([1e16, 1.0, -1e16, 1.0])
    assert float(np.cumsum(t)[-1]) == ((1e16 + 1.0) - 1e16) + 1.0


def test_bounds_hold_between_orders_on_a_larger_plane():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (120, 160), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    s, _, _, abs_sums, terms = Q.fast_ssim(a, b, want_map=False)
    n = (120 - 7) * (160 - 7)
    f = Q.fsum_ssim(terms, n)
    assert abs(s - f) <= Q.ssim_bound(abs_sums, 1)
    pairwise = (float(np.sum(terms[0])) / (64.0 * n)) * 100.0
    assert abs(pairwise - f) <= Q.fsum_bound(abs_sums, 1, n)


# ---- the edge tests' contents and shapes (tests/test_gpu_quality_edges.py) ---------------------------------

@pytest.mark.parametrize("H,W", [(16, 16), (9, 17)])
def test_fast_form_equals_the_literal_one_on_the_extremes(H, W):
    """All 255, 255 against 0, checkerboard against its inverse, constant against noise: the integer-moment form's
    largest sums and its negative windows."""
    rng = np.random.default_rng(H * W)
    for kind in range(len(E.EXTREMES)):
        for Cn in (1, 3):
            a, b = E.extreme_pair(kind, rng, H, W, Cn)
            ls, lm, lsc = Q.literal_ssim(a, b)
            fs, fm, fsc, _, _ = Q.fast_ssim(a, b)
            assert (bits(lm) == bits(fm)).all(), (kind, Cn)
            assert bits(lsc).tolist() == bits(fsc).tolist()
            assert bits(ls) == bits(fs)
            if kind == 0:
                assert ls == 100.0
            if kind == 2:  # every window holds 32 and 32: one value, the most negative there is
                m2, cv = 2.0 * 127.5 * 127.5, 64.0 * 127.5 * 127.5  # means 127.5; variances 64 * 127.5^2, covariance minus that
                want = ((m2 + Q.C1) * (2.0 * -cv + Q.C2)) / ((m2 + Q.C1) * (cv + cv + Q.C2))
                assert (bits(fm) == bits(want)).all() and want < -0.9999
                if (H, W) == (16, 16):  # (the frame's figure is a sequential sum: its last digits follow the window count)
                    assert ls == fs == -99.99437515819864
    a, b = E.extreme_pair(1, rng, H, W, 1)
    assert Q.mse_psnr(a, b)[0] == 65025.0


def test_unlike_channels_are_unlike():
    rng = np.random.default_rng(8)
    a, b = E.unlike_channels(rng, 3, 12, 10, 3)
    for f in range(3):
        roles = [(f + ch) % 3 for ch in range(3)]
        assert np.array_equal(a[f, ..., roles.index(0)], b[f, ..., roles.index(0)])
        assert np.array_equal(255 - a[f, ..., roles.index(1)], b[f, ..., roles.index(1)])
        scores = Q.fast_ssim(a[f], b[f])[2]
        assert scores[roles.index(0)] == 1.0 and scores[roles.index(1)] < -0.5 < scores[roles.index(2)] < 0.5
    a, b = E.unlike_channels(rng, 2, 12, 10, 1)
    assert np.abs(a[0].astype(int) - b[0]).max() <= 3 and np.abs(a[1].astype(int) - b[1]).max() > 100


def test_edge_shapes_straddle_the_kernel_constants():
    k = kernel_constants.quality()
    assert k["kSsimTileW"] == k["kQualBlock"] - 8 and k["kSsimTileH"] % 8 == 0
    tw, th = k["kSsimTileW"], k["kSsimTileH"]
    ww = [w - 7 for w in E.tile_edge_widths(k)]
    wh = [h - 7 for h in E.tile_edge_heights(k)]
    assert min(ww) == 1 and min(wh) == 1
    assert {tw - 1, tw, tw + 1, 2 * tw, 2 * tw + 1} <= set(ww)           # a tile less one, full, and one column over
    assert {w % tw for w in ww if w > tw} >= {1, 7, 8, 0}                # last tiles of 1, 7 and 8 windows, and full
    assert {th - 1, th, th + 1, 2 * th, 2 * th + 1} <= set(wh)
    assert {min(th, h) % 8 for h in wh} == set(range(8))                 # every exit phase of the unrolled row loop
    assert any(h > th and h % th == 1 for h in wh)                       # a tile of a single window row below a full one
    # at today's constants these are the lists the tests were written for
    if (tw, th) == (248, 32):
        assert [w + 7 for w in ww] == [8, 9, 15, 254, 255, 256, 262, 263, 503, 504]
        assert set(h + 7 for h in wh) >= {8, 14, 15, 16, 38, 39, 40, 71, 72}
    W, H, clamp = E.sse_clamp_plane(k)
    assert clamp == k["kSseMaxBlocks"] * k["kSseBytesPerBlock"] and clamp < W * H <= clamp + W and (W * H) % 16 == 0
    assert W < 65536 and H < 65536


def test_known_changes_have_the_stated_sum():
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, 300000, dtype=np.uint8)
    b, sse = E.known_changes(rng, a, 200000)
    d = a.astype(np.int64) - b.astype(np.int64)
    assert int((d * d).sum()) == sse and 900 < np.count_nonzero(d) < 1100
    assert d[0] and d[-1] and d[199999] and d[200000] and d[15] and d[16]


def test_kernel_constants_fail_loudly():
    text = "constexpr uint32_t kA = 256;\nconstexpr uint32_t kB = kA * 16u * 8u;  // c\nconstexpr uint32_t kC = kA - 8;\n"
    assert kernel_constants.parse_u32_constants(text, ("kA", "kB", "kC")) == {"kA": 256, "kB": 32768, "kC": 248}
    with pytest.raises(KeyError):
        kernel_constants.parse_u32_constants(text, ("kA", "kMissing"))
    with pytest.raises(KeyError):
        kernel_constants.parse_u32_constants("constexpr uint32_t kD = sizeof(int);", ("kD",))
    f = kernel_constants.framer()
    assert all(v > 0 for v in f.values()) and len(f) == 5


# ---- the library ------------------------------------------------------------------------------------------------

def test_library_exports_every_quality_symbol_and_the_table_matches():
    from adder_amd import quality
    hdr = open(os.path.join(ROOT, "include", "adder_quality.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(adder_quality_\w+)\s*\(", hdr))
    assert len(names) >= 6 and names == set(quality.SYMBOLS)
    L = quality.load()
    for n in names:
        assert hasattr(L, n), n


def test_params_struct_matches_the_header():
    from adder_amd import quality
    assert C.sizeof(quality.AdderQualityParams) == 16 and C.sizeof(quality.AdderQualityResult) == 32
    assert quality.AdderQualityParams.device_id.offset == 12


def test_create_without_a_device_reports_no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from adder_amd import quality, _native as N
    with pytest.raises(N.AdderHipError) as ei:
        quality.HipQuality(16, 16, 1, ssim=True)
    assert ei.value.code == N.E_NO_DEVICE
    # argument errors come first, device or not
    L = quality.load()
    h = C.c_void_p()
    for w, h_, ch, m in ((0, 8, 1, 7), (8, 8, 2, 7), (8, 8, 1, 0)):
        p = quality.AdderQualityParams(abi_version=1, width=w, height=h_, channels=ch, metrics=m)
        assert L.adder_quality_create(C.byref(p), C.byref(h)) == N.E_BAD_PARAMS
    p = quality.AdderQualityParams(abi_version=2, width=8, height=8, channels=1, metrics=7)
    assert L.adder_quality_create(C.byref(p), C.byref(h)) == N.E_BAD_PARAMS


def test_host_mirror_unchanged():
    from adder_amd import calculate_quality_metrics
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    mse, psnr = Q.mse_psnr(a, b)
    assert calculate_quality_metrics(a, b) == {"mse": mse, "psnr": psnr}
    assert calculate_quality_metrics(a, a) == {"mse": 1e-7, "psnr": 20.0 * math.log10(255.0) + 70.0}
