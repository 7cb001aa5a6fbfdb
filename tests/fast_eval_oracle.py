"""The definition include/adder_fast.h is checked against, written independently of csrc/adder_fast_logic.hpp (numpy):

  * dense FAST 9_16 by the literal ring walk of utils/cv.rs:56-212 (the threshold table, the opposite-pair quick
    rejects, the 25-step walk with its carried count and its k == 17 exit), the threshold a parameter, applied at
    every pixel -- vectorised over the pixels, step for step the same walk;
  * the score by brute force: the largest t in 0 .. 254 at which that walk says "feature";
  * strict 3x3 suppression (kept iff the score is above each of the 8 neighbours'; outside the plane counts as 0);
  * feature_precision_recall_accuracy (cv.rs:235-279) restated literally for one channel: hash sets and the y, x loop.
"""
import numpy as np

# cv.rs:25-30
CIRCLE3 = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
           (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
STREAK_SIZE = 9
BORDER = 3


def channel0(frame):
    """[H][W] or [H][W][C] -> the [H][W] plane the detectors read (cv.rs:61-67: channel 0)."""
    a = np.asarray(frame, np.uint8)
    return a if a.ndim == 2 else a[:, :, 0]


def _centres_and_rings(plane):
    """The candidates (cv.rs:61 is_border(.., 3)) of an [H][W] plane, flattened in raster order:
    -> ys, xs, centre [N] int16, ring [16][N] int16."""
    h, w = plane.shape
    if h <= 2 * BORDER or w <= 2 * BORDER:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, np.int16), np.zeros((16, 0), np.int16)
    ys, xs = np.meshgrid(np.arange(BORDER, h - BORDER), np.arange(BORDER, w - BORDER), indexing="ij")
    ys, xs = ys.ravel(), xs.ravel()
    p = plane.astype(np.int16)
    ring = np.stack([p[ys + b, xs + a] for a, b in CIRCLE3])
    return ys, xs, p[ys, xs], ring


def walk(centre, ring, threshold):
    """is_feature (cv.rs:65-211) for N pixels at once: centre [N], ring [16][N] int16 -> bool [N]."""
    t = int(threshold)
    n = centre.shape[0]
    diff = ring - centre[None, :]
    tab = np.where(diff < -t, 1, np.where(diff > t, 2, 0)).astype(np.uint8)  # THRESHOLD_TABLE
    result = np.zeros(n, bool)
    d = tab[0] | tab[8]
    done = d == 0                                   # cv.rs:93
    for a in (2, 4, 6):
        d = d & (tab[a] | tab[a + 8])
    done |= d == 0                                  # cv.rs:115
    for a in (1, 3, 5, 7):
        d = d & (tab[a] | tab[a + 8])
    for bit, sign in ((1, -1), (2, 1)):             # the dark streak, then the bright one
        active = ~done & ((d & bit) > 0)
        vt = centre + sign * t
        count = np.zeros(n, np.int32)
        for k in range(16 + STREAK_SIZE):
            x = ring[k % 16]
            hit = (x < vt) if sign < 0 else (x > vt)
            count = np.where(hit, count + 1, 0)
            won = active & hit & (count == STREAK_SIZE)
            result |= won
            done |= won
            active &= ~won
            if k == 17:                             # "can't be a streak long enough": return Ok(false)
                bail = active & ~hit
                done |= bail
                active &= ~bail
    return result


def dense_fast(plane, threshold):
    """-> bool [H][W]: the literal walk at every pixel."""
    plane = channel0(plane)
    out = np.zeros(plane.shape, bool)
    ys, xs, c, ring = _centres_and_rings(plane)
    if len(ys):
        out[ys, xs] = walk(c, ring, threshold)
    return out


def score_plane(plane, threshold):
    """-> uint8 [H][W]: for a pixel the walk calls a feature at `threshold`, the largest t in 0 .. 254 at which it
    still does (every t is tried); 0 elsewhere."""
    plane = channel0(plane)
    out = np.zeros(plane.shape, np.uint8)
    ys, xs, c, ring = _centres_and_rings(plane)
    if not len(ys):
        return out
    sel = walk(c, ring, threshold)
    ys, xs, c, ring = ys[sel], xs[sel], c[sel], ring[:, sel]
    best = np.full(len(ys), -1, np.int32)
    for t in range(255):
        best[walk(c, ring, t)] = t
    assert (best >= 0).all()
    out[ys, xs] = best
    return out


def suppress(score):
    """Strict 3x3 suppression -> bool [H][W]."""
    s = np.asarray(score).astype(np.int32)
    h, w = s.shape
    pad = np.zeros((h + 2, w + 2), np.int32)
    pad[1:-1, 1:-1] = s
    keep = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= s > pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return keep


def from_score(score, nonmax):
    """A frame's score plane -> (mask uint8 [H][W], score, xy uint32 [kept] in raster order)."""
    mask = suppress(score) if nonmax else score > 0
    ys, xs = np.nonzero(mask)
    return mask.astype(np.uint8), score, (xs.astype(np.uint32) | (ys.astype(np.uint32) << 16))


def detect(frame, threshold, nonmax):
    """One frame -> (mask, score, xy).  (score > 0 is dense_fast(frame, threshold): score_plane scores the pixels the
    walk accepts, and never with less than the threshold, which is at least 1.)"""
    return from_score(score_plane(frame, threshold), nonmax)


def stack(results):
    """Per-frame (mask, score, xy) -> (mask [n][H][W], score [n][H][W], xy of all frames, counts int64 [n])."""
    return (np.stack([r[0] for r in results]), np.stack([r[1] for r in results]),
            np.concatenate([r[2] for r in results]).astype(np.uint32), np.array([len(r[2]) for r in results], np.int64))


def detect_frames(frames, threshold, nonmax):
    """[n][H][W] or [n][H][W][C] -> (mask [n][H][W], score [n][H][W], xy of all frames, counts int64 [n])."""
    return stack([detect(f, threshold, nonmax) for f in frames])


def precision_recall_accuracy(gt_mask, pred_mask):
    """cv.rs:235-279 for one channel: gt the detector's key points, prediction the event-driven feature set."""
    gt_mask, pred_mask = np.asarray(gt_mask), np.asarray(pred_mask)
    h, w = gt_mask.shape
    gt_hash = {(int(x), int(y)) for y, x in zip(*np.nonzero(gt_mask))}
    prediction = {(int(x), int(y)) for y, x in zip(*np.nonzero(pred_mask))}
    tp = fp = tn = fnn = 0
    for y in range(h):
        for x in range(w):
            coord = (x, y)
            if coord in prediction:
                if coord in gt_hash:
                    tp += 1
                else:
                    fp += 1
            elif coord in gt_hash:
                fnn += 1
            else:
                tn += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = np.float64(tp) / np.float64(tp + fp)
        recall = np.float64(tp) / np.float64(tp + fnn)
        accuracy = np.float64(tp + tn) / np.float64(tp + tn + fp + fnn)
    return {"tp": tp, "fp": fp, "tn": tn, "fn": fnn, "gt_count": len(gt_hash), "pred_count": len(prediction),
            "precision": float(precision), "recall": float(recall), "accuracy": float(accuracy)}
