"""Test images for the PNG encoder tests (numpy only)."""
import numpy as np


def gradient_noise(h, w, c, seed=0, sigma=3.0):
    """smooth gradients plus gaussian noise of `sigma`: what a camera frame looks like to a scanline predictor"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([40.0 + 0.55 * x + 0.3 * y + 25 * k + 20 * np.sin(x / 17.0 + k) * np.cos(y / 23.0) for k in range(c)], 2)
    return np.clip(base + rng.normal(0, sigma, (h, w, c)), 0, 255).round().astype(np.uint8)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else b if pb <= pc else c


def five_winners(w=32, c=3, seed=5):
    """(9, w, c) uint8 in which every filter type wins at least one row under the smallest-sum-of-absolute-values heuristic:
    row 0 bytes near 0 as signed values (none), row 2 a ramp under an unrelated row (sub), row 4 a copy of row 3 (up), row 6 exactly the
    mean of left and above (average), row 8 exactly the Paeth predictor; rows 1, 3, 5, 7 are uniform noise."""
    rng = np.random.default_rng(seed)
    r = w * c
    rows = np.zeros((9, r), np.int64)
    rows[0] = rng.choice([0, 1, 255], r)
    for y in (1, 3, 5, 7):
        rows[y] = rng.integers(0, 256, r)
    rows[2] = (np.arange(r) // c * 5 + 30) % 256
    rows[4] = rows[3]
    for i in range(r):
        rows[6, i] = ((rows[6, i - c] if i >= c else 0) + rows[5, i]) >> 1
    for i in range(r):
        rows[8, i] = _paeth(rows[8, i - c] if i >= c else 0, rows[7, i], rows[7, i - c] if i >= c else 0)
    return rows.astype(np.uint8).reshape(9, w, c)
