"""For whoever has OpenCV: compare `cv2.resize(img, (w, h), interpolation=cv2.INTER_CUBIC)` with this project's definition of it
(`dataset.cubic_tables` + the integer passes, restated in numpy below; `ops.resize_cubic_u8` computes exactly that on the device).

The definition is OpenCV's scalar fixed-point path, which rounds exact ties (v mod 2^22 == 2^21) up.  A SIMD build of OpenCV runs the
vertical pass of most columns in float and rounds to nearest-even, so it may differ on those ties, by 1.  This prints, per image,
the largest difference, the share of differing samples, and how many of the differing samples are exact ties of the definition.
Nobody has run it against a real cv2 build yet.  It needs cv2 and does not fall back without it; no test depends on it.

    python tools/compare_cv2_resize.py [image files ...]          # without files: seeded random and smooth images
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def resize_cubic_u8(img: np.ndarray, size):
    """img uint8 (H, W, C) -> (out uint8 (h, w, C), v int64): the project's definition, from the product's tables"""
    from eavsr_amd.dataset import cubic_tables
    H, W = img.shape[:2]
    h, w = size
    (yo, yk), (xo, xk) = cubic_tables(H, h), cubic_tables(W, w)
    src = img.astype(np.int64)
    hor = sum(xk[:, j].astype(np.int64)[None, :, None] * src[:, np.clip(xo + (j - 1), 0, W - 1), :] for j in range(4))
    v = sum(yk[:, j].astype(np.int64)[:, None, None] * hor[np.clip(yo + (j - 1), 0, H - 1)] for j in range(4))
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8), v


def main():
    import cv2      # required: this tool measures cv2
    print("cv2", cv2.__version__, "| SIMD / dispatch:", [ln.strip() for ln in cv2.getBuildInformation().splitlines() if "Baseline" in ln or "Dispatched" in ln])
    images = []
    for path in sys.argv[1:]:
        img = cv2.imread(path, cv2.IMREAD_COLOR)
        if img is None:
            raise SystemExit(f"{path}: not an image cv2 can read")
        images.append((path, img))
    if not images:
        rng = np.random.default_rng(0)
        yy, xx = np.mgrid[0:720, 0:1280]
        smooth = np.stack([127.5 + 127.5 * np.sin(xx / (9.0 + 4 * c)) * np.cos(yy / (7.0 + 3 * c)) for c in range(3)], -1)
        images = [("random 720 x 1280", rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8)),
                  ("smooth 720 x 1280", smooth.round().astype(np.uint8)),
                  ("random 203 x 517", rng.integers(0, 256, (203, 517, 3), dtype=np.uint8))]
    for name, img in images:
        H, W = img.shape[:2]
        for h, w in {(H // 4, W // 4), (H // 2, W // 2), (max(1, (H * 10) // 41), max(1, (W * 10) // 37))}:
            ref = cv2.resize(img, (w, h), interpolation=cv2.INTER_CUBIC).reshape(h, w, -1)
            got, v = resize_cubic_u8(img, (h, w))
            diff = np.abs(ref.astype(np.int64) - got.astype(np.int64))
            ties = (v & ((1 << 22) - 1)) == (1 << 21)
            print(f"{name}: {H} x {W} -> {h} x {w}: max |cv2 - definition| {int(diff.max())}, differing {100.0 * float((diff > 0).mean()):.4f} % "
                  f"of {diff.size} samples ({int(((diff > 0) & ties).sum())} of the {int((diff > 0).sum())} are exact ties; {int(ties.sum())} ties in all)")


if __name__ == "__main__":
    main()
