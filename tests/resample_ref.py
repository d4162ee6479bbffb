"""The oracle of the LR synthesis (ops.resize_cubic_u8, csrc/resize_cubic.hip, dataset.cubic_tables): OpenCV's `resize` for CV_8U,
INTER_CUBIC, restated from its definition with scalar numpy arithmetic.  It builds its OWN tables (nothing of eavsr_amd is imported)
and returns the int64 accumulator beside the image, so that tests can count exact ties and saturated samples.

One axis, `src` samples in and `dst` out, output index d:
    scale = 1.0 / (dst / src)                     float64 (OpenCV inverts the inverse scale)
    f = float32((d + 0.5) * scale - 0.5);  s = floor(f);  x = float32(f - s)
    A = -0.75f, float32, left to right:
      c0 = ((A*(x+1) - 5*A)*(x+1) + 8*A)*(x+1) - 4*A      c1 = ((A+2)*x - (A+3))*x*x + 1
      c2 = ((A+2)*(1-x) - (A+3))*(1-x)*(1-x) + 1          c3 = 1 - c0 - c1 - c2
    k_j = saturate_int16(round_half_even(c_j * 2048))      (the sum is not corrected to 2048)
    taps s-1, s, s+1, s+2, each clamped into [0, src-1]
Image: hor = sum_j kx_j * src (exact), v = sum_j ky_j * hor, out = clamp((v + 2^21) >> 22, 0, 255), arithmetic shift."""
import math

import numpy as np

F32 = np.float32


def axis_tables(src: int, dst: int):
    """(ofs: list of dst ints, coef: list of dst 4-tuples of ints), one output sample at a time"""
    scale = 1.0 / (dst / src)
    A = F32(-0.75)
    ofs, coef = [], []
    for d in range(dst):
        f = F32((d + 0.5) * scale - 0.5)
        s = math.floor(float(f))
        x = F32(f - F32(s))
        x1 = F32(x + F32(1))
        c0 = F32(F32(F32(F32(F32(F32(A * x1) - F32(F32(5) * A)) * x1) + F32(F32(8) * A)) * x1) - F32(F32(4) * A))
        a2, a3 = F32(A + F32(2)), F32(A + F32(3))
        c1 = F32(F32(F32(F32(F32(a2 * x) - a3) * x) * x) + F32(1))
        xm = F32(F32(1) - x)
        c2 = F32(F32(F32(F32(F32(a2 * xm) - a3) * xm) * xm) + F32(1))
        c3 = F32(F32(F32(F32(1) - c0) - c1) - c2)
        ks = []
        for c in (c0, c1, c2, c3):
            k = int(np.rint(F32(c * F32(2048))))       # np.rint: half to even
            ks.append(max(-32768, min(32767, k)))
        ofs.append(int(s))
        coef.append(tuple(ks))
    return ofs, coef


def _taps(src: int, dst: int):
    ofs, coef = axis_tables(src, dst)
    idx = np.asarray([[min(max(s - 1 + j, 0), src - 1) for j in range(4)] for s in ofs], np.int64)      # (dst, 4)
    return idx, np.asarray(coef, np.int64)


def resize_cubic_u8(img: np.ndarray, size):
    """img uint8 (..., H, W) planes -> (out uint8 (..., h, w), v int64 (..., h, w)), size = (h, w)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim >= 2
    H, W = img.shape[-2:]
    h, w = size
    xi, xk = _taps(W, w)
    yi, yk = _taps(H, h)
    src = img.astype(np.int64)
    hor = np.zeros(img.shape[:-1] + (w,), np.int64)
    for j in range(4):
        hor += xk[:, j] * src[..., :, xi[:, j]]
    assert np.abs(hor).max(initial=0) < 2 ** 31
    v = np.zeros(img.shape[:-2] + (h, w), np.int64)
    for j in range(4):
        v += yk[:, j][:, None] * hor[..., yi[:, j], :]
    assert np.abs(v).max(initial=0) < 2 ** 31 - 2 ** 21
    out = np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    return out, v


def counts(v: np.ndarray):
    """(exact ties, samples clamped to 0, samples clamped to 255) of an accumulator"""
    q = (v + (1 << 21)) >> 22
    return int(((v & ((1 << 22) - 1)) == (1 << 21)).sum()), int((q < 0).sum()), int((q > 255).sum())
