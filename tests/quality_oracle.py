"""Restatements of the reference's quality metrics (adder-codec-rs/src/utils/cv.rs:306-430) for the tests.

literal_*: cv.rs line by line -- every 8x8 window at stride 1 in row-major order, the means and the (co)variances as
sequential f64 sums, the window's expression in the reference's order, the channel score as sequential sums.  Slow:
small planes only.

fast_*: the integer-moment form -- box sums of x, y, xy, x^2, y^2 from integral images, from which the reference's
means, variances and covariance follow exactly, the same last f64 operations, and the channel's sequential
sum through np.cumsum (np.add.accumulate adds left to right; np.sum would add pairwise).  Equal to literal_* bit for bit
(tests/test_quality_cpu.py), fast enough for 1080p and 4K.
"""
import math

import numpy as np

K1, K2, L = 0.01, 0.03, 255
C1 = (K1 * float(L)) * (K1 * float(L))
C2 = (K2 * float(L)) * (K2 * float(L))
WIN = 8


def _planes(a):
    a = np.asarray(a)
    return a[:, :, None] if a.ndim == 2 else a


def mse_psnr(original, reconstructed):
    """cv.rs:317-330 / 337-351: (mse with 0 -> 1e-7, psnr)."""
    a = _planes(original).astype(np.int64)
    b = _planes(reconstructed).astype(np.int64)
    err = 0.0
    for d in (a - b).ravel().tolist():  # (exact integers: the order does not matter, kept sequential anyway)
        err += float(d * d)
    mse = err / float(a.size)
    if mse == 0.0:
        mse = 0.0000001
    return mse, 20.0 * math.log10(255.0) - 10.0 * math.log10(mse)


# ---- literal ----------------------------------------------------------------------------------------------------

def literal_window(wx, wy):
    """ssim_for_window (cv.rs:394-404): wx, wy lists of 64 ints in the window's element order."""
    mx = 0.0
    for v in wx:
        mx += float(v)
    mx = mx / float(len(wx))
    my = 0.0
    for v in wy:
        my += float(v)
    my = my / float(len(wy))

    def cov(xs, mx_, ys, my_):
        s = 0.0
        for x, y in zip(xs, ys):
            s += (float(x) - mx_) * (float(y) - my_)
        return s
    vx = cov(wx, mx, wx, mx)
    vy = cov(wy, my, wy, my)
    c = cov(wx, mx, wy, my)
    counter = (2.0 * mx * my + C1) * (2.0 * c + C2)
    denominator = (mx * mx + my * my + C1) * (vx + vy + C2)
    return counter / denominator


def literal_channel(pa, pb):
    """-> (score, [r of every window, row-major]) of one channel plane [H][W] (cv.rs:370-385)."""
    H, W = pa.shape
    rs = []
    for y in range(H - WIN + 1):
        for x in range(W - WIN + 1):
            rs.append(literal_window(pa[y:y + WIN, x:x + WIN].ravel().tolist(), pb[y:y + WIN, x:x + WIN].ravel().tolist()))
    num = 0.0
    for r in rs:
        num += r * float(WIN * WIN)
    den = 0.0
    for _ in rs:
        den += float(WIN * WIN)
    return (num / den if den else math.nan), rs


def literal_ssim(original, reconstructed):
    """-> (ssim, map [C][H-7][W-7] as float64, per-channel scores)."""
    a, b = _planes(original), _planes(reconstructed)
    H, W, C = a.shape
    scores, maps = [], []
    for ch in range(C):
        s, rs = literal_channel(a[:, :, ch], b[:, :, ch])
        scores.append(s)
        maps.append(np.array(rs, dtype=np.float64).reshape(max(H - 7, 0), max(W - 7, 0)))
    tot = 0.0
    for s in scores:
        tot += s
    return (tot / float(C)) * 100.0, np.stack(maps), scores


# ---- vectorised ---------------------------------------------------------------------------------------------------

def _box8(v):
    """8x8 box sums of an int64 plane [H][W] -> [H-7][W-7]."""
    ii = np.zeros((v.shape[0] + 1, v.shape[1] + 1), np.int64)
    ii[1:, 1:] = v.cumsum(0).cumsum(1)
    return ii[8:, 8:] - ii[:-8, 8:] - ii[8:, :-8] + ii[:-8, :-8]


def fast_channel_map(pa, pb):
    """Every window's r of one channel plane, bit-equal to literal_channel's."""
    x = pa.astype(np.int64)
    y = pb.astype(np.int64)
    sx, sy = _box8(x), _box8(y)
    sxx, syy, sxy = _box8(x * x), _box8(y * y), _box8(x * y)
    m2 = (2 * sx * sy).astype(np.float64) / 4096.0            # 2 mx my
    cv2 = (64 * sxy - sx * sy).astype(np.float64) / 32.0      # 2 cov
    mm = (sx * sx + sy * sy).astype(np.float64) / 4096.0      # mx^2 + my^2
    vv = (64 * sxx - sx * sx + 64 * syy - sy * sy).astype(np.float64) / 64.0  # vx + vy
    return ((m2 + C1) * (cv2 + C2)) / ((mm + C1) * (vv + C2))


def fast_ssim(original, reconstructed, want_map=True):
    """-> (ssim, map [C][H-7][W-7] or None, per-channel scores, per-channel sum of |r|, per-channel list of 64 r)."""
    a, b = _planes(original), _planes(reconstructed)
    H, W, C = a.shape
    if H < WIN or W < WIN:
        return math.nan, (np.zeros((C, 0, 0)) if want_map else None), [math.nan] * C, [0.0] * C, [np.zeros(0)] * C
    maps, scores, abs_sums, terms = [], [], [], []
    for ch in range(C):
        r = fast_channel_map(a[:, :, ch], b[:, :, ch])
        t = (r * 64.0).ravel()
        num = float(np.cumsum(t)[-1])           # the reference's sequential sum
        den = float(np.cumsum(np.full(t.size, 64.0))[-1])
        scores.append(num / den)
        abs_sums.append(float(np.abs(r).sum()))
        terms.append(t)
        if want_map:
            maps.append(r)
    tot = 0.0
    for s in scores:
        tot += s
    return (tot / float(C)) * 100.0, (np.stack(maps) if want_map else None), scores, abs_sums, terms


def ssim_bound(abs_sums, C):
    """|device - sequential| allowed for a frame's SSIM: the first-order bound of the two summation orders,
    100 * 2^-52 * sum over channels and windows of |r| / C, plus a few ulp of 100 for the last operations."""
    return 100.0 * 2.0 ** -52 * sum(abs_sums) / C + 4 * math.ulp(100.0)


def fsum_ssim(terms, windows):
    """The frame's SSIM from correctly rounded channel sums (math.fsum of the 64 r terms)."""
    tot = 0.0
    for t in terms:
        tot += math.fsum(t.tolist()) / (64.0 * windows)
    return (tot / float(len(terms))) * 100.0


def fsum_bound(abs_sums, C, windows):
    """2^-40 * sum |64 r| on each channel's sum, carried through / (64 N), / C and * 100."""
    return 100.0 * 2.0 ** -40 * sum(abs_sums) / (windows * C) + 4 * math.ulp(100.0)
