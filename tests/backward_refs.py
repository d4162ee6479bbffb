"""Float64 restatements of the operations whose backward kernels the training step runs (csrc/backward.hip,
backward_dcn.hip, dcn_bwd.hip), and the input builders of tests/test_hip_backward_kernels.py.

Every reference is the plain operation -- the oracle's function or the torch op itself -- so that CPU autograd through it in
float64 is the gradient the kernels must reproduce.  tests/test_backward_refs_host.py checks, without a GPU, that each one run
forward equals the float32 oracle / aten op it restates."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import eavsr_oracle as O

Tensor = torch.Tensor
F64 = torch.float64


def gen(seed: int) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def randn64(seed: int, *shape, scale: float = 1.0) -> Tensor:
    """float64 normal values already rounded to float32: the GPU gets .float() of them, the reference the same operands"""
    return (torch.randn(*shape, generator=gen(seed), dtype=F64) * scale).float().double()


def uniform64(seed: int, lo: float, hi: float, *shape) -> Tensor:
    return (lo + (hi - lo) * torch.rand(*shape, generator=gen(seed), dtype=F64)).float().double()


# ------------------------------------------------------------------------------------------ references
def resize_ac(x: Tensor, size, scale: float, pre: Optional[Tensor] = None, post: Optional[Tensor] = None) -> Tensor:
    """scale * interpolate(x [+ pre], size, bilinear, align_corners=True) [+ post]  (ops.resize_bilinear_ac)"""
    t = x if pre is None else x + pre
    y = F.interpolate(t, size=tuple(size), mode="bilinear", align_corners=True) * scale
    return y if post is None else y + post


def flow_warp(x: Tensor, flow: Tensor, flow2: Optional[Tensor] = None) -> Tensor:
    """grid_sample on the normalised grid, zeros padding, align_corners=True (ops.flow_warp)"""
    return O.flow_warp(x, flow if flow2 is None else flow + flow2)


def affine(heads: Tensor, D: int, with_mask: bool) -> Tuple[Tensor, Optional[Tensor]]:
    """heads (n, 6D | 15D, h, w): transform 4D, translation 2D [, mask logits 9D] -> (offset, sigmoid(logits))  (ops.affine_offsets)"""
    off = O.affine_offsets(heads[:, :4 * D], heads[:, 4 * D:6 * D], D)
    return off, (torch.sigmoid(heads[:, 6 * D:15 * D]) if with_mask else None)


def gconv(x: Tensor, w: Tensor, b: Optional[Tensor], act: Optional[str], slope: float = 0.2) -> Tensor:
    """3x3 convolution with one output channel per group (cpg = w.shape[1] inputs each), padding 1 [, LeakyReLU]  (ops.gconv3x3)"""
    y = F.conv2d(x, w, b, 1, 1, 1, int(w.shape[0]))
    return F.leaky_relu(y, slope) if act == "lrelu" else y


def pyramid(x: Tensor) -> Tuple[Tensor, Tensor]:
    """interpolate x0.5 and x0.25, bilinear, align_corners=False  (ops.pyramid)"""
    return O.feature_pyramid(x)


def rcab_tail(r: Tensor, x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor) -> Tensor:
    """r * sigmoid(W2 relu(W1 mean_hw(r) + b1) + b2) + x  (autograd.rcab_tail; w1 (cr, c, 1, 1), w2 (c, cr, 1, 1))"""
    cr, c = int(w1.shape[0]), int(w1.shape[1])
    m = r.mean(dim=(2, 3))
    hid = torch.relu(m @ w1.reshape(cr, c).t() + b1)
    s = torch.sigmoid(hid @ w2.reshape(c, cr).t() + b2)
    return r * s[:, :, None, None] + x


def dcnv2(x, offset, mask, weight, bias, dg: int) -> Tensor:
    return O.dcnv2(x, offset, mask, weight, bias, 1, 1, 1, 1, dg)


# ------------------------------------------------------------------------------------------ sample positions
FRAC = (0.05, 0.95)     # fractional parts of every sample position: never within 0.05 of an integer, where the derivative
                        # w.r.t. the position is one-sided and float32 rounding could pick the other side
REGIONS = ("inside", "edge", "far", "mixed")


def _axis_targets(g: torch.Generator, mode: Tensor, size: int, base: Tensor) -> Tensor:
    """positions along one axis: mode 0 all corners inside, 1 one pixel outside the low edge (-1 + u: only corner 1 valid), 2 one
    pixel outside the high edge (size - 1 + u: only corner 0 valid), 3 far outside (|flow| > size + 4: the kernel's clamp)"""
    u = FRAC[0] + (FRAC[1] - FRAC[0]) * torch.rand(mode.shape, generator=g, dtype=F64)
    inside = torch.randint(0, max(size - 1, 1), mode.shape, generator=g).to(F64) + u
    sign = torch.where(torch.rand(mode.shape, generator=g) < 0.5, -1.0, 1.0).to(F64)
    far = base + sign * (size + 5.0 + 10.0 * u)
    return torch.where(mode == 0, inside, torch.where(mode == 1, u - 1.0, torch.where(mode == 2, size - 1.0 + u, far)))


def warp_flow(seed: int, n: int, h: int, w: int, region: str) -> Tensor:
    """(n, 2, h, w) float64 flow, rounded to float32, whose sample positions (pixel + flow) lie in `region`:
    inside  -- all four corners inside the image;
    edge    -- within one pixel outside an edge in x, y or both (only one corner column / row valid; x = w - 1 + u among them);
    far     -- |flow| > size + 4 in x, y or both (every corner invalid; the kernel clamps the position to [-4, size + 4]);
    mixed   -- every pixel draws one of the three."""
    g = gen(seed)
    shape = (n, h, w)
    if region == "inside":
        mx = my = torch.zeros(shape, dtype=torch.long)
    elif region == "edge":
        mx, my = torch.randint(0, 3, shape, generator=g), torch.randint(0, 3, shape, generator=g)
        both_in = (mx == 0) & (my == 0)
        mx = torch.where(both_in, 1 + torch.randint(0, 2, shape, generator=g), mx)
    elif region == "far":
        pick = torch.randint(0, 3, shape, generator=g)     # 0: x far, 1: y far, 2: both
        mx = torch.where(pick != 1, 3, torch.randint(0, 3, shape, generator=g))
        my = torch.where(pick != 0, 3, torch.randint(0, 3, shape, generator=g))
    elif region == "mixed":
        mx, my = torch.randint(0, 4, shape, generator=g), torch.randint(0, 4, shape, generator=g)
        keep = torch.rand(shape, generator=g) < 0.5        # half of the pixels sample well inside
        mx, my = torch.where(keep, 0, mx), torch.where(keep, 0, my)
    else:
        raise ValueError(region)
    gy, gx = torch.meshgrid(torch.arange(h, dtype=F64), torch.arange(w, dtype=F64), indexing="ij")
    gx, gy = gx.expand(shape), gy.expand(shape)
    tx, ty = _axis_targets(g, mx, w, gx), _axis_targets(g, my, h, gy)
    return torch.stack((tx - gx, ty - gy), 1).float().double()


def positions(flow: Tensor) -> Tuple[Tensor, Tensor]:
    """(tx, ty) = pixel + flow, (n, h, w) each"""
    n, _, h, w = flow.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=F64), torch.arange(w, dtype=F64), indexing="ij")
    return gx + flow[:, 0], gy + flow[:, 1]


def no_valid_corner(flow: Tensor) -> Tensor:
    """(n, h, w) bool: the sample at pixel + flow has no corner inside the image (its d(flow) is exactly zero)"""
    h, w = flow.shape[2:]
    tx, ty = positions(flow)
    return (tx <= -1) | (tx >= w) | (ty <= -1) | (ty >= h)


def reached(flow: Tensor) -> Tensor:
    """(n, h, w) bool: pixels that are a valid corner of at least one sample (everything else gets an exactly zero dx)"""
    n, _, h, w = flow.shape
    tx, ty = positions(flow)
    x0, y0 = torch.floor(tx).long(), torch.floor(ty).long()
    hit = torch.zeros(n, h * w, dtype=torch.bool)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            for b in range(n):
                hit[b, (yy[b][ok[b]] * w + xx[b][ok[b]])] = True
    return hit.view(n, h, w)


def dcn_offsets(seed: int, n: int, dg: int, h: int, w: int, sigma: float) -> Tensor:
    """DCNv2 offsets (n, 18 dg, h, w): an integer part of spread ~sigma plus a fraction in FRAC, so that every sample position
    (integer tap + offset) keeps its fractional part away from integers and from the validity bounds -1 < p < size"""
    g = gen(seed)
    shape = (n, dg * 18, h, w)
    whole = torch.floor(torch.randn(shape, generator=g, dtype=F64) * sigma)
    u = FRAC[0] + (FRAC[1] - FRAC[0]) * torch.rand(shape, generator=g, dtype=F64)
    return (whole + u).float().double()
