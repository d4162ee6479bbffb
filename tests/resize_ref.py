"""The numpy restatement of `eavsr_amd.resize.resize_frames`: rows first, then columns, plain loops over the taps in
increasing order, a tap whose weight is zero skipped and never multiplied.  In float32 every product and every sum is rounded on its
own (numpy has no fused multiply-add), which is what csrc/resize_aa.hip computes: the GPU tests compare raw bits.  The float64 version
runs the same loops on the same (float32) tables in double."""
import os
import re

import numpy as np

from eavsr_amd.resize import axis_tables, tmp_row


def _rows(src, idx, wgt, dtype):
    """(H, X) -> (out, X) along axis 0: t[o, :] = acc over k: acc = 0; if w[o, k] != 0: acc = acc + w[o, k] * src[idx[o, k], :]"""
    out = np.empty((idx.shape[0], src.shape[1]), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for o in range(idx.shape[0]):
            acc = np.zeros(src.shape[1], dtype)
            for k in range(idx.shape[1]):
                w = dtype(wgt[o, k])
                if w != 0:
                    acc = acc + w * src[idx[o, k]]
            out[o] = acc
    return out


def resize_plane(plane, size, dtype=np.float32):
    """one (H, W) plane -> (oh, ow) in `dtype` arithmetic"""
    plane = np.asarray(plane, dtype)
    iv, wv = axis_tables(plane.shape[0], size[0])
    ih, wh = axis_tables(plane.shape[1], size[1])
    t = _rows(plane, iv, wv, dtype)
    return np.ascontiguousarray(_rows(np.ascontiguousarray(t.T), ih, wh, dtype).T)


def resize(x, size, dtype=np.float32):
    """(.., H, W) -> (.., oh, ow): `resize_plane` of every plane.  size == (H, W) is the input itself, as the op returns it."""
    x = np.asarray(x, dtype)
    if tuple(size) == tuple(x.shape[-2:]):
        return x
    flat = x.reshape((-1,) + x.shape[-2:])
    out = np.stack([resize_plane(p, size, dtype) for p in flat], 0)
    return out.reshape(x.shape[:-2] + tuple(size))


def touched(shape, size, y, x):
    """the outputs (oh, ow) bool whose non-zero taps read sample (y, x) of a plane of `shape`, from the tables alone"""
    iv, wv = axis_tables(shape[0], size[0])
    ih, wh = axis_tables(shape[1], size[1])
    rows = ((iv == y) & (wv != 0)).any(axis=1)
    cols = ((ih == x) & (wh != 0)).any(axis=1)
    return rows[:, None] & cols[None, :]


# ------------------------------------------------------------------------ csrc/resize_aa.hip, transcribed: addresses, not arithmetic
def kernel_constants():
    """the constexpr ints of csrc/resize_aa.hip by name"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eavsr_amd", "csrc", "resize_aa.hip")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;", f.read())}


def piece_columns(W, ow, taps, c=None):
    """`cols` of eavsr_resize_aa_f32: the output columns of one piece of the horizontal pass"""
    c = c or kernel_constants()
    cols = min(c["kMaxCols"], c["kLdsTable"] // taps)
    room = c["kLdsRow"] - c["kSpanMargin"] - taps - 1
    return min(cols, room * ow // W + 1)


def transcription(mem, base, strides, shape, size, threads=256):
    """Both kernels as they index memory, on a flat float32 array `mem` whose element 0 sits on a 16-byte boundary: the source is
    (N, C, H, W) = shape at element `base` with element strides (sN, sC, sH) (last stride 1).  Returns (out (N, C, oh, ow), stats):
    stats counts the float4 and the scalar loads of the vertical pass, the pieces of the horizontal pass and its widest span.  Every
    access is checked against the buffer it belongs to."""
    c = kernel_constants()
    N, C, H, W = shape
    sN, sC, sH = strides
    oh, ow = size
    iv, wv = axis_tables(H, oh)
    ih, wh = axis_tables(W, ow)
    Kv, Kh = iv.shape[1], ih.shape[1]
    Wt = tmp_row(W)
    rows = N * C * oh
    tmp = np.full(rows * Wt, np.nan, np.float32)
    written = np.zeros(rows * Wt, bool)
    stats = {"vec": 0, "scalar": 0, "pieces": 0, "span": 0}
    f32 = np.float32
    quads = (W + 6) // 4
    blocks = -(-quads // threads)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rows):
            p, o = divmod(r, oh)
            plane = base + (p // C) * sN + (p % C) * sC
            phase = plane & 3
            for q in range(blocks * threads):
                x0 = 4 * q - phase
                if x0 >= W:
                    continue
                full = x0 >= 0 and x0 + 3 < W
                acc = [f32(0)] * 4
                for k in range(Kv):
                    w = wv[o, k]
                    if w != 0:
                        off = int(min(max(iv[o, k], 0), H - 1)) * sH
                        row = plane + off
                        if full and off & 3 == 0:
                            assert (row + x0) % 4 == 0, "a float4 load off its boundary"
                            v = [mem[row + x0 + j] for j in range(4)]
                            stats["vec"] += 1
                        else:
                            v = [mem[row + x0 + j] if 0 <= x0 + j < W else f32(0) for j in range(4)]
                            stats["scalar"] += sum(0 <= x0 + j < W for j in range(4))
                        acc = [f32(a + f32(w * vj)) for a, vj in zip(acc, v)]
                at = r * Wt + 4 * q
                if full:
                    assert at % 4 == 0
                for j in range(4):
                    if 0 <= x0 + j < W:
                        assert at + j < (r + 1) * Wt and not written[at + j]
                        tmp[at + j], written[at + j] = acc[j], True
        cols = piece_columns(W, ow, Kh, c)
        assert cols >= 1 and 2 * Kh * cols <= 2 * c["kLdsTable"]
        out = np.full((rows, ow), np.nan, np.float32)
        for p0 in range(0, ow, cols):
            nc = min(cols, ow - p0)
            tab_i = np.clip(ih[p0:p0 + nc], 0, W - 1)
            lo, hi = int(tab_i.min()), int(tab_i.max())
            assert hi - lo + 1 <= c["kLdsRow"], "the span of a piece does not fit the staged row"
            span = min(hi - lo + 1, c["kLdsRow"])
            stats["pieces"] += 1
            stats["span"] = max(stats["span"], span)
            for r in range(rows):
                plane = base + ((r // oh) // C) * sN + ((r // oh) % C) * sC
                at = r * Wt + (plane & 3) + lo
                assert written[at:at + span].all(), "the horizontal pass stages a sample the vertical pass did not write"
                st = tmp[at:at + span]
                for j in range(nc):
                    a = f32(0)
                    for k in range(Kh):
                        w = wh[p0 + j, k]
                        if w != 0:
                            a = f32(a + f32(w * st[tab_i[j, k] - lo]))
                    out[r, p0 + j] = a
    return out.reshape(N, C, oh, ow), stats
