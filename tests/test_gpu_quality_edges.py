"""The quality kernels (csrc/adder_quality.hip) past the edges of their own launch geometry: SSIM tiles that hold one
window column or row, a last tile of 7 and of 8 windows, every exit phase of the row loop; contents at which the packed
halves and the 32-bit expressions reach their maxima; calls of several launch groups (f0 != 0); a frame past the SSE
grid clamp; pointers off the 16-byte grid; planes one window thick.  The shapes follow the constants of
csrc/adder_quality_kernels.h (tests/kernel_constants.py).  Every comparison is bit for bit against
tests/quality_oracle.py and adder_amd.calculate_quality_metrics; the frame's SSIM within Q.ssim_bound / Q.fsum_bound
(test_gpu_quality._check_frames)."""
import functools
import math

import numpy as np
import pytest

import kernel_constants
import quality_edge_cases as E
import quality_oracle as Q
from test_gpu_quality import _check_frames, _cuda, bits

pytestmark = pytest.mark.gpu

K = kernel_constants.quality()
GUARD = 64          # sentinel elements on each side of a map
SENTINEL = -7.0


def _hip():
    import adder_amd
    return adder_amd


def _results(got):
    """The device's dicts -> the bit patterns of [n][mse, psnr, ssim]."""
    return bits(np.array([[g["mse"], g["psnr"], g["ssim"]] for g in got]).reshape(len(got), 3))


def _run_guarded(A, q, d_a, d_b, n):
    """compute_device with the map inside a larger tensor: -> (dicts, map [n][C][H-7][W-7] as numpy).  Asserts that
    the elements on both sides of the map are untouched and that the frame's numbers do not depend on the map."""
    import torch
    shape = q.map_shape(n)
    elems = int(np.prod(shape))
    buf = torch.full((elems + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    dmap = buf[GUARD:GUARD + elems]
    dmap.fill_(math.nan)  # (a window the kernel leaves out differs from every value of the restatement)
    got = q.compute_device(d_a, d_b, ssim_map=dmap)
    edges = torch.cat([buf[:GUARD], buf[GUARD + elems:]])
    assert edges.numel() == 2 * GUARD and bool((edges == SENTINEL).all()), "the map was written out of its bounds"
    plain = q.compute_device(d_a, d_b)
    assert (_results(plain) == _results(got)).all(), "the frame's numbers depend on the map pointer"
    return got, dmap.cpu().numpy().reshape(shape)


def _check(A, a, b):
    n, H, W, Cn = a.shape
    q = A.HipQuality(W, H, Cn, ssim=True)
    got, dmap = _run_guarded(A, q, _cuda(a), _cuda(b), n)
    _check_frames(A, a, b, got, dmap)


# ---- a. tile edges, b. map bounds ---------------------------------------------------------------------------------

@pytest.mark.parametrize("W", E.tile_edge_widths(K))
def test_tile_edges_and_map_bounds(W):
    """Windows per row on the edges of the tile's 248 columns x window rows on the edges of its 32 rows and of the
    unrolled row loop, C = 1 and 3, two frames a call: unlike channels, then the four extreme contents."""
    A = _hip()
    rng = np.random.default_rng(1000 + W)
    for H in E.tile_edge_heights(K):
        for Cn in (1, 3):
            _check(A, *E.unlike_channels(rng, 2, H, W, Cn))
            _check(A, *E.extreme_frames(rng, (0, 1), H, W, Cn))
            _check(A, *E.extreme_frames(rng, (2, 3), H, W, Cn))


# ---- c. launch groups -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,Cn,n", [(9, 8, 1, E.GRID_ROWS_MAX + 6), (8, 9, 3, 2 * (E.GRID_ROWS_MAX // 3) + 3)])
def test_launch_groups_past_the_first(W, H, Cn, n):
    """More frames than one launch group holds (two groups, three groups): frame f of the call is base pair f % 61, so
    a group that restarts at frame 0 -- f0 dropped in the SSE, the SSIM or the combine kernel -- repeats the wrong
    frames (61 is prime against 65535 and 21845)."""
    import torch
    A = _hip()
    rng = np.random.default_rng(77 + Cn)
    base_a, base_b = E.unlike_channels(rng, 61, H, W, Cn)
    q = A.HipQuality(W, H, Cn, ssim=True)
    assert n > E.GRID_ROWS_MAX // Cn
    base_got, base_map = _run_guarded(A, q, _cuda(base_a), _cuda(base_b), 61)
    _check_frames(A, base_a, base_b, base_got, base_map)
    idx = np.arange(n) % 61
    group = E.GRID_ROWS_MAX // Cn
    assert all(idx[g] != 0 and (base_a[idx[g]] != base_a[0]).any() for g in range(group, n, group))
    a, b = base_a[idx], base_b[idx]
    want, want_map = _results(base_got)[idx], bits(base_map[idx])
    dmap = torch.full(q.map_shape(n), math.nan, dtype=torch.float64, device="cuda")
    got = q.compute_device(_cuda(a), _cuda(b), ssim_map=dmap)
    assert (_results(got) == want).all(), np.flatnonzero((_results(got) != want).any(axis=1))[:8]
    assert (bits(dmap.cpu().numpy()) == want_map).all()
    hmap = np.full(q.map_shape(n), math.nan)
    host = q.compute(a, b, ssim_map=hmap)
    assert (_results(host) == want).all(), np.flatnonzero((_results(host) != want).any(axis=1))[:8]
    assert (bits(hmap) == want_map).all()


# ---- d. the SSE grid clamp, e. pointers off the 16-byte grid ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _clamp_case():
    """The plane just past the SSE clamp: a random frame, the same with known changes, the expected result."""
    A = _hip()
    W, H, clamp = E.sse_clamp_plane(K)
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, W * H, dtype=np.uint8)
    b, sse = E.known_changes(rng, a, clamp)
    mse = float(sse) / float(a.size)
    return W, H, a, b, {"mse": mse, "psnr": A.calculate_psnr(mse)}


def test_sse_past_the_grid_clamp():
    """One frame of more bytes than kSseMaxBlocks blocks cover in a pass: the blocks stride.  The expected SSE is the
    closed-form sum of the known changes; all 255 against all 0 is the largest sum a frame of this size has."""
    import torch
    A = _hip()
    W, H, a, b, want = _clamp_case()
    assert W * H > K["kSseMaxBlocks"] * K["kSseBytesPerBlock"] and (W * H) % 16 == 0
    q = A.HipQuality(W, H, 1, ssim=False)
    assert q.compute_device(_cuda(a), _cuda(b)) == [want]
    assert q.compute_device(_cuda(b), _cuda(a)) == [want]
    hi = torch.full((W * H,), 255, dtype=torch.uint8, device="cuda")
    lo = torch.zeros(W * H, dtype=torch.uint8, device="cuda")
    assert q.compute_device(hi, lo) == [{"mse": 65025.0, "psnr": A.calculate_psnr(65025.0)}]


def _at_offset(x, off):
    """x as a contiguous CUDA view whose first byte sits `off` bytes past a 16-byte boundary."""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(x).reshape(-1))
    buf = torch.empty(flat.numel() + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == off and view.is_contiguous()
    return view


def test_pointers_off_the_16_byte_grid():
    """Frames of a multiple of 16 bytes behind a pointer that is not: the SSE takes the bytewise path, the SSIM its
    usual one, and every number and window equals the aligned call's."""
    import torch
    A = _hip()
    rng = np.random.default_rng(41)
    W, H, n = 64, 48, 2
    a, b = E.unlike_channels(rng, n, H, W, 1)
    q = A.HipQuality(W, H, 1, ssim=True)
    ref, ref_map = _run_guarded(A, q, _cuda(a), _cuda(b), n)
    _check_frames(A, a, b, ref, ref_map)
    for oa, ob in ((1, 0), (0, 1), (1, 1), (15, 0), (0, 15), (15, 15), (1, 15)):
        got, dmap = _run_guarded(A, q, _at_offset(a, oa), _at_offset(b, ob), n)
        assert (_results(got) == _results(ref)).all(), (oa, ob)
        assert (bits(dmap) == bits(ref_map)).all(), (oa, ob)
    # the plane past the SSE clamp, both inputs one byte off: the bytewise path strides too
    W, H, a, b, want = _clamp_case()
    assert A.HipQuality(W, H, 1, ssim=False).compute_device(_at_offset(a, 1), _at_offset(b, 1)) == [want]


def test_frames_that_start_misaligned_inside_an_aligned_batch():
    """243-byte frames: frames 1 .. 4 of an aligned batch start off the 16-byte grid."""
    A = _hip()
    rng = np.random.default_rng(43)
    a, b = E.unlike_channels(rng, 5, 9, 9, 3)
    assert a[0].size % 16 != 0
    _check(A, a, b)
    ea, eb = E.extreme_frames(rng, (0, 1, 2, 3, 2), 9, 9, 3)
    _check(A, ea, eb)


# ---- f. one window thick ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(8, 5000), (5000, 8)])
def test_planes_one_window_thick(W, H):
    """One tile column of many tile rows, and many tile columns of one window row each."""
    A = _hip()
    rng = np.random.default_rng(W)
    q = A.HipQuality(W, H, 1, ssim=True)
    assert max(q.map_shape(1)[2:]) > 4 * max(K["kSsimTileW"], K["kSsimTileH"]) and min(q.map_shape(1)[2:]) == 1
    for Cn in (1, 3):
        _check(A, *E.unlike_channels(rng, 2, H, W, Cn))
        _check(A, *E.extreme_frames(rng, (2, 3), H, W, Cn))


@pytest.mark.parametrize("W,H", [(300, 7), (7, 300)])
def test_planes_without_a_window(W, H):
    """No 8 x 8 window: NaN SSIM (the reference's 0 / 0), MSE and PSNR exact."""
    A = _hip()
    rng = np.random.default_rng(H)
    for Cn in (1, 3):
        a, b = E.unlike_channels(rng, 3, H, W, Cn)
        got = A.HipQuality(W, H, Cn, ssim=True).compute_device(_cuda(a), _cuda(b))
        assert all(math.isnan(g["ssim"]) for g in got)
        _check_frames(A, a, b, got)
