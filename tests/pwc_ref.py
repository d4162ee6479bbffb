"""CPU restatement of PWC-Net (models/pwc_net.py), BaseModel.estimate and BaseModel.get_backwarp (models/base_model.py:294-354),
written from their description: functional, over a state_dict with the reference's key names.  It is the checker of the HIP
path (eavsr_amd.pwc) and, for the cost volume, of the golden recipe (tests/golden/gen_golden_pwc.py), whose reference
correlation is four CUDA kernels with no CPU branch."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

CH = [16, 32, 64, 96, 128, 196]
FLT_BACKWARP = {5: 0.625, 4: 1.25, 3: 2.5, 2: 5.0}
LEVEL_NAMES = {1: "One", 2: "Two", 3: "Thr", 4: "Fou", 5: "Fiv", 6: "Six"}


def correlation(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(n, 81, h, w): channel (dy+4)*9 + (dx+4) = mean over channels of a[y, x] * b[y+dy, x+dx], zero outside the image (no
    activation)"""
    n, c, h, w = a.shape
    bp = F.pad(b, (4, 4, 4, 4))
    out = a.new_zeros((n, 81, h, w))
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            out[:, (dy + 4) * 9 + (dx + 4)] = (a * bp[:, :, 4 + dy:4 + dy + h, 4 + dx:4 + dx + w]).sum(1) / c
    return out


def _lrelu(x):
    return F.leaky_relu(x, 0.1)


def grid_warp(x: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """x (n, c, h, w) and a ones channel sampled (bilinear, zeros, align_corners=False) at the linspace(-1 + 1/w, 1 - 1/w) grid
    plus the flow in normalised units (flow / ((w - 1) / 2)): (n, c + 1, h, w), the last channel unthresholded"""
    n, _, h, w = flow.shape
    gx = torch.linspace(-1.0 + 1.0 / w, 1.0 - 1.0 / w, w).view(1, 1, 1, w).expand(n, 1, h, w)
    gy = torch.linspace(-1.0 + 1.0 / h, 1.0 - 1.0 / h, h).view(1, 1, h, 1).expand(n, 1, h, w)
    fx = flow[:, 0:1] / ((x.shape[3] - 1.0) / 2.0)
    fy = flow[:, 1:2] / ((x.shape[2] - 1.0) / 2.0)
    grid = torch.cat([gx + fx, gy + fy], 1).permute(0, 2, 3, 1)
    xo = torch.cat([x, x.new_ones((n, 1, h, w))], 1)
    return F.grid_sample(xo, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def threshold(ones: torch.Tensor) -> torch.Tensor:
    return (ones > 0.999).to(ones.dtype)


def _conv(sd, key, x, stride=1, dil=1, act=True):
    y = F.conv2d(x, sd[key + ".weight"], sd[key + ".bias"], stride=stride, padding=dil, dilation=dil)
    return _lrelu(y) if act else y


def pwc_forward(sd, first: torch.Tensor, second: torch.Tensor, corr=correlation) -> torch.Tensor:
    """PWC-Net's flow (n, 2, H/4, W/4) for H, W multiples of 64"""
    def extract(x):
        feats = []
        for level in range(1, 7):
            k = "netExtractor.net" + LEVEL_NAMES[level]
            x = _conv(sd, k + ".0", x, stride=2)
            x = _conv(sd, k + ".2", x)
            x = _conv(sd, k + ".4", x)
            feats.append(x)
        return feats

    f1, f2 = extract(first), extract(second)
    flow = feat = None
    for level in range(6, 1, -1):
        k = "net" + LEVEL_NAMES[level]
        a, b = f1[level - 1], f2[level - 1]
        if level == 6:
            feat = _lrelu(corr(a, b))
        else:
            up_flow = F.conv_transpose2d(flow, sd[k + ".netUpflow.weight"], sd[k + ".netUpflow.bias"], stride=2, padding=1)
            up_feat = F.conv_transpose2d(feat, sd[k + ".netUpfeat.weight"], sd[k + ".netUpfeat.bias"], stride=2, padding=1)
            warped = grid_warp(b, up_flow * FLT_BACKWARP[level])
            b_w = warped[:, :-1] * threshold(warped[:, -1:])
            feat = torch.cat([_lrelu(corr(a, b_w)), a, up_flow, up_feat], 1)
        for name in ["netOne", "netTwo", "netThr", "netFou", "netFiv"]:
            feat = torch.cat([_conv(sd, f"{k}.{name}.0", feat), feat], 1)
        flow = _conv(sd, k + ".netSix.0", feat, act=False)
    r = feat
    for i, dil in zip(range(0, 13, 2), [1, 2, 4, 8, 16, 1, 1]):
        r = _conv(sd, f"netRefiner.netMain.{i}", r, dil=dil, act=i < 12)
    return flow + r


def estimate(sd, first, second, corr=correlation):
    n, _, h, w = first.shape
    hp, wp = int(math.ceil(h / 64.0) * 64), int(math.ceil(w / 64.0) * 64)
    p1 = F.interpolate(first, size=(hp, wp), mode="bilinear", align_corners=False)
    p2 = F.interpolate(second, size=(hp, wp), mode="bilinear", align_corners=False)
    flow = 20.0 * F.interpolate(pwc_forward(sd, p1, p2, corr), size=(h, w), mode="bilinear", align_corners=False)
    flow[:, 0] *= float(w) / float(wp)
    flow[:, 1] *= float(h) / float(hp)
    return flow


def get_backwarp(sd, lr, hr, scale, corr=correlation):
    """(hr_align, mask, ones, flow): ones is the warped ones channel before the threshold, flow the LR flow"""
    with torch.no_grad():
        small = F.interpolate(hr, scale_factor=1.0 / scale, mode="bilinear", align_corners=True)
        flow = estimate(sd, lr, small, corr)
        up = F.interpolate(flow, scale_factor=scale, mode="nearest") * scale
        out = grid_warp(hr, up)
        ones = out[:, -1:].clone()
        mask = threshold(ones)
        return out[:, :-1] * mask, mask, ones, flow
