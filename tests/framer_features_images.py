"""Images for the corner-test comparisons of tests/test_framer_features_cpu.py (helper; holds no test)."""
import numpy as np

import clips


def images():
    rng = np.random.default_rng(17)
    yield rng.integers(0, 256, (40, 52), dtype=np.uint8)
    yield (rng.integers(0, 2, (40, 52)) * 200 + rng.integers(0, 30, (40, 52))).astype(np.uint8)
    yield (rng.integers(0, 3, (33, 47, 3)) * 100 + rng.integers(0, 40, (33, 47, 3))).astype(np.uint8)
    for k in range(4):
        yield clips.make_clip("corners", 1, 48, 64, 1, seed=20 + k)[0, :, :, 0]
    img = np.full((20, 20), 100, np.uint8)  # the thresholds are strict: +-30 is no corner, +-31 is one
    img[10:, 10:] = 130
    yield img
    img = img.copy()
    img[10:, 10:] = 131
    yield img
    yield np.zeros((7, 7), np.uint8)
    yield np.zeros((6, 9), np.uint8)
