"""Seeded planes for the dense FAST detector and its scoring (tests/test_fast_eval_cpu.py, tests/test_gpu_fast_eval.py).

CASES: name -> Case(frames [n][H][W] uint8, thresholds to run).  CENSUS: name -> what the case is there for, as counts
at (threshold 30, no suppression / suppression) the CPU test asserts against the oracle -- so that a change of the
generator that loses a case's point fails there."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "frames thresholds")


def _rng(tag):
    return np.random.default_rng([20260321, tag])


def constant(w=40, h=30, v=77):
    return np.full((1, h, w), v, np.uint8)


def noise(w, h, seed, n=1):
    """Uniform noise: many corners."""
    return _rng(seed).integers(0, 256, (n, h, w)).astype(np.uint8)


def noise_levels(w, h, seed, n=1):
    """Noise over five levels: many corners with equal scores next to each other (suppression ties)."""
    return (_rng(seed).integers(0, 5, (n, h, w)) * 63).astype(np.uint8)


def squares(w, h, seed, n=1, count=4, bg=20, fg=200):
    """Filled squares on a flat background: real corners."""
    r = _rng(seed)
    out = np.full((n, h, w), bg, np.uint8)
    for f in range(n):
        for _ in range(count):
            s = int(r.integers(5, 12))
            x, y = int(r.integers(0, max(w - s, 1))), int(r.integers(0, max(h - s, 1)))
            out[f, y:y + s, x:x + s] = fg
    return out


def moving_square(w=64, h=48, n=3, size=9, bg=30, fg=150):
    """A shaded square (so that its corners' scores differ and suppression keeps some) that moves from frame to frame."""
    out = np.full((n, h, w), bg, np.uint8)
    shade = 6 * np.add.outer(np.arange(size), np.arange(size))
    for f in range(n):
        x, y = 6 + 7 * f, 5 + 4 * f
        out[f, y:y + size, x:x + size] = fg + shade
    return out


def noise_and_squares(w, h, seed, n=1):
    """What the size sweeps of the GPU test use: mild noise (corners of every score) under a few squares."""
    r = _rng(seed)
    out = r.integers(60, 140, (n, h, w)).astype(np.uint8)
    sq = squares(w, h, seed + 1, n, count=max(2, w * h // 1500), bg=0, fg=230)
    return np.where(sq > 0, sq, out).astype(np.uint8)


def equal_pair(w=24, h=16):
    """Two adjacent pixels of 200 on 100: each is a corner of score 99 (its whole ring is 100 darker), nothing else is;
    strict suppression keeps neither."""
    out = np.full((1, h, w), 100, np.uint8)
    out[0, 8, 10] = out[0, 8, 11] = 200
    return out


def edge_corners(w=23, h=17):
    """Single pixels of 250 on 40 in the first and last candidate column and row (x = 3, x = W - 4, y = 3, y = H - 4)
    -- corners -- and one column / row further out (x = 2, y = H - 3) -- not looked at."""
    out = np.full((1, h, w), 40, np.uint8)
    for x, y in ((3, 3), (w - 4, 3), (3, h - 4), (w - 4, h - 4), (2, 8), (11, h - 3)):
        out[0, y, x] = 250
    return out


def extremes(w=30, h=20):
    """All 0 / 255: a 255 pixel on 0 and a 0 pixel on 255 both reach the score 254."""
    out = np.zeros((2, h, w), np.uint8)
    out[0, 9, 8] = 255
    out[0, 5, 20] = 255
    out[1] = 255
    out[1, 10, 15] = 0
    return out


CASES = {
    "constant": Case(constant(), (1, 30, 255)),
    "noise": Case(noise(67, 45, 1, n=2), (1, 30, 255)),
    "noise_levels": Case(noise_levels(53, 41, 2), (1, 30)),
    "squares": Case(squares(64, 48, 3, n=2), (1, 30)),
    "moving_square": Case(moving_square(), (30,)),
    "noise_and_squares": Case(noise_and_squares(70, 37, 4), (1, 30, 255)),
    "equal_pair": Case(equal_pair(), (30, 99, 100)),
    "edge_corners": Case(edge_corners(), (30,)),
    "extremes": Case(extremes(), (1, 30, 254, 255)),
    "no_candidates_6x9": Case(noise(6, 9, 5), (30,)),
    "no_candidates_9x6": Case(noise(9, 6, 6), (30,)),
    "one_candidate_7x7": Case(np.where(np.arange(49).reshape(1, 7, 7) == 24, 0, 200).astype(np.uint8), (30,)),
}

# name -> (kept without suppression, kept with it) at threshold 30, summed over the frames: exact where the case is
# built to a count, a lower bound ("min") where it is there for being busy
CENSUS = {
    "constant": {"plain": 0, "nonmax": 0},
    "noise": {"plain_min": 100, "nonmax_min": 30},
    "noise_levels": {"plain_min": 40, "ties_min": 5},
    "squares": {"plain_min": 16},
    "moving_square": {"plain_min": 12, "nonmax_min": 3},
    "equal_pair": {"plain": 2, "nonmax": 0, "ties_min": 1},
    "edge_corners": {"plain": 4, "nonmax": 4},
    "extremes": {"plain": 3, "nonmax": 3, "max_score": 254},
    "no_candidates_6x9": {"plain": 0, "nonmax": 0},
    "no_candidates_9x6": {"plain": 0, "nonmax": 0},
    "one_candidate_7x7": {"plain": 1, "nonmax": 1},
}


def predictions(truth, seed=7):
    """truth: bool / 0-1 [H][W] -> name -> uint8 [H][W] prediction plane (nonzero = predicted; the values vary, as a
    caller's plane may hold any nonzero byte)."""
    truth = np.asarray(truth) != 0
    r = _rng(seed)
    some = r.integers(0, 8, truth.shape) == 0
    return {
        "empty": np.zeros(truth.shape, np.uint8),
        "full": r.integers(1, 256, truth.shape).astype(np.uint8),
        "equal": (truth * r.integers(1, 256, truth.shape)).astype(np.uint8),
        "disjoint": (~truth & some).astype(np.uint8) * 255,
        "mixed": ((truth & (r.integers(0, 2, truth.shape) == 0)) | some).astype(np.uint8) * 128,
    }
