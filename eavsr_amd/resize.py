"""Output at any target size: the antialiased bicubic resize of fp32 frames on the device.

The definition is MATLAB's `imresize(I, [oh ow])` -- Keys' cubic with a = -0.5, stretched (antialiased) along an axis that shrinks,
symmetric border -- the "Bicubic" of SR tables and the BI degradation of the public benchmarks.  `axis_tables` builds one axis of it
on the host in float64 (the general form of `niqe.resize_tables`, which stays as it is: one factor, no upscaling, fp64 weights);
`resize_frames` applies the tables of both axes with one HIP op, csrc/resize_aa.hip, rows first, then columns, every fp32 operation
rounded on its own, so that tests/resize_ref.py restates the result bit for bit.

What is NOT claimed: the values have not been compared with MATLAB or with any package (none is available where this was written);
and the fp32 path on frames in [0, 1] is not MATLAB's uint8 path, which computes in double on 0 .. 255 and rounds to a byte.
torch's `F.interpolate(mode="bicubic", antialias=True)` uses a = -0.75: a timing baseline, never a parity one.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np

from .niqe import _cubic

MAX_TAPS = 64                        # csrc/resize_aa.hip kMaxTaps: about out >= length / 15.5


def axis_tables(length: int, out: int) -> Tuple[np.ndarray, np.ndarray]:
    """`axis_tables64` with the weights rounded once to float32: what the device reads"""
    idx, w = axis_tables64(length, out)
    return idx, np.ascontiguousarray(w.astype(np.float32))


def axis_tables64(length: int, out: int) -> Tuple[np.ndarray, np.ndarray]:
    """One axis of `imresize(I, [.. out ..])` for `length` samples: (idx int32 (out, taps), weight float64 (out, taps)), idx 0-based.
    scale = out / length in float64, s = min(scale, 1).  Output x = 1 .. out sits at u = x / scale + 0.5 (1 - 1 / scale); the kernel is
    stretched to the width 4 / s; its ceil(width) + 2 taps start at left = floor(u - width / 2) and weigh s k(s (u - i)), each row
    divided by its float64 sum; indices outside 1 .. length are reflected symmetrically (.. 2, 1, 1, 2 ..); columns that are zero for
    every output are dropped (`axis_tables` then rounds the weights once to float32).  Rows of the kept columns still hold single
    zeros: the op skips them.  More than MAX_TAPS taps is a ValueError."""
    if isinstance(length, bool) or isinstance(out, bool) or not isinstance(length, (int, np.integer)) or not isinstance(out, (int, np.integer)):
        raise ValueError(f"axis_tables: length {length!r} -> {out!r}: whole numbers of samples")
    length, out = int(length), int(out)
    if length < 1 or out < 1:
        raise ValueError(f"axis_tables: length {length} -> {out}: at least one sample on both sides")
    scale = np.float64(out) / np.float64(length)
    s = min(scale, np.float64(1.0))
    x = np.arange(1, out + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1.0 - 1.0 / scale)
    width = 4.0 / s
    left = np.floor(u - width / 2.0)
    taps = int(math.ceil(width)) + 2
    ind = left[:, None] + np.arange(taps, dtype=np.float64)[None, :]
    w = s * _cubic(s * (u[:, None] - ind))
    w = w / w.sum(axis=1, keepdims=True)
    aux = np.concatenate([np.arange(length), np.arange(length - 1, -1, -1)])
    idx = aux[np.mod(ind.astype(np.int64) - 1, 2 * length)]
    keep = np.any(w != 0.0, axis=0)
    if int(keep.sum()) > MAX_TAPS:
        raise ValueError(f"axis_tables: {length} -> {out} samples needs {int(keep.sum())} taps, at most {MAX_TAPS} "
                         f"(about out >= length / 15.5): resize in two steps")
    return np.ascontiguousarray(idx[:, keep], np.int32), np.ascontiguousarray(w[:, keep], np.float64)


def check_out_size(value, who: str = "out_size") -> Optional[Tuple[int, int]]:
    """None, or (H, W) from a pair of positive ints or the text form "1080x1920" (rows x columns); anything else is a ValueError
    that opens with `<who>=<value>: `"""
    if value is None:
        return None
    if isinstance(value, str):
        parts = value.split("x")
        if len(parts) != 2 or not all(p.isdigit() for p in parts):
            raise ValueError(f"{who}={value!r}: output pixels as '1080x1920' (rows x columns)")
        value = (int(parts[0]), int(parts[1]))
    if (not isinstance(value, (tuple, list)) or len(value) != 2
            or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in value)):
        raise ValueError(f"{who}={value!r}: (rows, columns), '1080x1920' or None")
    h, w = int(value[0]), int(value[1])
    if h < 1 or w < 1 or h > (1 << 24) or w > (1 << 24):
        raise ValueError(f"{who}={value!r}: each side is 1 .. 2^24 pixels")
    return h, w


def out_size_option(opt=None) -> Optional[Tuple[int, int]]:
    """None or (H, W): the size `harness.super_resolve` and `EAVSRPModel.forward` (outside training) resize the SR frames to --
    `opt.out_size` ((rows, columns) or "1080x1920"), falling back to the environment where the options do not carry it
    (EAVSR_OUT_SIZE=1080x1920), None -- the network's own s h x s w, no launch -- where neither does.  Not among the reference's
    options."""
    from .segments import read_option
    return read_option(opt, "out_size", "EAVSR_OUT_SIZE", check_out_size, check_out_size)


# the device copies of `axis_tables(length, out)`: {(length, out, device): [idx, weight, uploading stream, streams recorded]}.  A
# function of the sizes alone (no parameter behind them: not a WeightCache), but held to the same stream order: the upload is a
# blocking copy on the caller's stream -- complete when it returns, so no other stream ever waits for it -- and a stream that reads
# the tables for the first time is recorded with the allocator, so that an evicted table is not handed out under a reader's feet.
_TABLES: Dict = {}
_TABLES_MAX = 64


def clear_device_tables() -> None:
    """drop the tables cached on the device"""
    _TABLES.clear()


def _tables_on(length: int, out: int, device):
    import torch
    key = (length, out, str(device))
    hit = _TABLES.get(key)
    if hit is None:
        idx, wgt = axis_tables(length, out)                  # ValueError above MAX_TAPS, before anything is launched
        if len(_TABLES) >= _TABLES_MAX:
            _TABLES.clear()
        hit = _TABLES[key] = [torch.from_numpy(idx).to(device), torch.from_numpy(wgt).to(device),
                              torch.cuda.current_stream(device).cuda_stream, set()]
    elif not torch.cuda.is_current_stream_capturing():
        cur = torch.cuda.current_stream(device)
        if cur.cuda_stream != hit[2] and cur.cuda_stream not in hit[3]:
            hit[3].add(cur.cuda_stream)
            hit[0].record_stream(cur)
            hit[1].record_stream(cur)
    return hit[0], hit[1]


def tmp_row(w: int) -> int:
    """floats of one row of the row pass's intermediate (include/eavsr_hip.h): W samples behind a phase of at most 3, in whole quads"""
    return (int(w) + 6) & ~3


def resize_frames(x, size, out=None):
    """fp32 frames on the device, (N, C, H, W) or (n, k, C, H, W) -> fp32 (.., oh, ow), size = (oh, ow): `imresize(I, [oh ow])` of every
    plane as `axis_tables` defines it, rows first, then columns:

        t[o, x] = acc over the taps k of the vertical table, in increasing k:  acc = 0.0f;  if wv[o, k] != 0: acc = acc + wv[o, k] * src[iv[o, k], x]
        y[o, p] = the same along x on t with the horizontal table

    every product and sum rounded to fp32 on its own; a zero weight is skipped, never multiplied (a non-finite pixel reaches exactly
    the outputs whose non-zero taps read it); nothing is clamped -- `ops.rgb8` / `ops.frame_metrics` downstream clamp.  Any batch,
    channel and row strides are taken as they are (a cropped view costs nothing); a source whose last stride is not 1, or whose two
    leading dimensions of five do not fold into one, is copied first.  size == (H, W) returns `x` itself (copied into `out` if given)
    with no launch.  `out`: a contiguous fp32 tensor of the result's shape on the same device (returned).  Two launches on the
    current stream, whatever N C is; the tables of a (length, out, device) are cached on the device after a blocking upload on that
    stream, so a warm call is graph-capturable.  Two calls agree bit for bit."""
    import torch
    from . import ops
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"resize_frames: expected a tensor, got {type(x)}")
    if not x.is_cuda:
        raise RuntimeError(f"resize_frames: tensor is on {x.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if x.dtype != torch.float32 or x.dim() not in (4, 5):
        raise ValueError(f"resize_frames: fp32 (N, C, H, W) or (n, k, C, H, W) frames, got {x.dtype} {tuple(x.shape)}")
    size = check_out_size(tuple(size) if isinstance(size, (tuple, list)) else size, "resize_frames: size")
    if size is None:
        raise ValueError("resize_frames: size=None: (rows, columns)")
    oh, ow = size
    lead = tuple(int(v) for v in x.shape[:-2])
    H, W = int(x.shape[-2]), int(x.shape[-1])
    if min(lead + (H, W)) < 1:
        raise ValueError(f"resize_frames: empty frames {tuple(x.shape)}")
    shape = lead + (oh, ow)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape
                            or not out.is_contiguous() or out.device != x.device):
        raise ValueError(f"resize_frames: out: a contiguous fp32 {shape} tensor on {x.device}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))} on {getattr(out, 'device', None)}")
    if (oh, ow) == (H, W):
        if out is None:
            return x
        out.copy_(x)
        return out
    x = x.detach()
    if W > 1 and x.stride(-1) != 1:
        x = x.contiguous()
    if x.dim() == 5 and lead[0] > 1 and lead[1] > 1 and x.stride(0) != lead[1] * x.stride(1):
        x = x.contiguous()
    if x.dim() == 5:
        n, c = lead[0] * lead[1], lead[2]
        s_n, s_c = (x.stride(1) if lead[1] > 1 else x.stride(0)), x.stride(2)
    else:
        n, c = lead
        s_n, s_c = x.stride(0), x.stride(1)
    s_h = x.stride(-2)
    iv, wv = _tables_on(H, oh, x.device)
    ih, wh = _tables_on(W, ow, x.device)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    ops._chk(out, "out")
    tmp = torch.empty((n * c * oh, tmp_row(W)), device=x.device, dtype=torch.float32)
    kv, kh = int(iv.shape[1]), int(ih.shape[1])
    st = ops._stream(x)
    planes = float(n * c)
    # algorithmic bytes: the source read once, the intermediate written and read, the result written
    ops._launch("resize_aa", 2.0 * planes * (oh * W * kv + oh * ow * kh), 4.0 * planes * (H * W + 2 * oh * W + oh * ow), x,
                lambda: ops.lib().eavsr_resize_aa_f32(x.data_ptr(), int(s_n), int(s_c), int(s_h), n, c, H, W, iv.data_ptr(), wv.data_ptr(), kv,
                                                      ih.data_ptr(), wh.data_ptr(), kh, tmp.data_ptr(), out.data_ptr(), oh, ow, st),
                "resize_aa")
    return out
