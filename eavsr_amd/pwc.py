"""PWC-Net (models/pwc_net.py) and the validity mask of the late-training phase (models/base_model.py:294-354) on HIP kernels.

From epoch `opt.npost` on, the reference's training forward (models/eavsrp_model.py:85-97) estimates for every frame the flow from
the LR frame to the downscaled HR frame with a frozen PWC-Net, warps the HR frame by it and multiplies the SR output by the
thresholded warped "ones" channel, so that HR content that moved out of frame stops contributing gradient.

`PWCNET` has the reference's module tree (its state_dict keys are those of models/pwc_net.py), but its forward runs only the
eavsr_pwc_* entry points (csrc/pwc.hip): no ATen convolution, grid_sample, interpolate or cat.  The decoder's dense
concatenations are never materialised: level L keeps ONE buffer (2N, intCurrent + 448, h, w) in the reference's concatenation
order -- [0:32] netFiv, [32:96] netFou, [96:192] netThr, [192:320] netTwo, [320:448] netOne, then [volume(81), first(C), upflow(2),
upfeat(2)] (level 6: the volume only) -- and every dense convolution reads the tail slice and writes the slice in front of it.
The extractor runs once over the 2N stacked images (first, then second) and writes its level-L output straight into the
`first` channels of that buffer, all 2N rows; the decoder works on rows [0:N], rows [N:2N] hold the second image's features.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch
import torch.nn as nn

from . import ops

Tensor = torch.Tensor

# feature channels of extractor levels 1..6, and the flow multiplier of the decoder's backwarp at levels 2..5 (pwc_net.py:117)
_CH = [16, 32, 64, 96, 128, 196]
_FLT_BACKWARP = {5: 0.625, 4: 1.25, 3: 2.5, 2: 5.0}
# channels of the decoder's dense convolutions, netOne .. netFiv (pwc_net.py:119-152), and where each writes in the level buffer
_DENSE = [128, 128, 96, 64, 32]
_DENSE_TOP = 448


def _current(level: int) -> int:
    """intCurrent of Decoder(level) (pwc_net.py:101-104): volume [+ first features + upflow + upfeat]"""
    return 81 if level == 6 else 81 + _CH[level - 1] + 2 + 2


def _seq(*convs):
    layers = []
    for i, (cin, cout, dil) in enumerate(convs):
        layers.append(nn.Conv2d(cin, cout, 3, 1, dil, dilation=dil))
        if i < len(convs) - 1 or cout != 2:
            layers.append(nn.LeakyReLU(0.1))
    return nn.Sequential(*layers)


class _Extractor(nn.Module):
    def __init__(self):
        super().__init__()
        cins = [3] + _CH[:-1]
        for name, cin, c in zip(["netOne", "netTwo", "netThr", "netFou", "netFiv", "netSix"], cins, _CH):
            seq = _seq((cin, c, 1), (c, c, 1), (c, c, 1))
            seq[0].stride = (2, 2)
            setattr(self, name, seq)

    def levels(self):
        return [self.netOne, self.netTwo, self.netThr, self.netFou, self.netFiv, self.netSix]


class _Decoder(nn.Module):
    def __init__(self, level: int):
        super().__init__()
        self.level = level
        cur = _current(level)
        if level < 6:
            self.netUpflow = nn.ConvTranspose2d(2, 2, 4, 2, 1)
            self.netUpfeat = nn.ConvTranspose2d(_current(level + 1) + _DENSE_TOP, 2, 4, 2, 1)
            self.fltBackwarp = _FLT_BACKWARP[level]
        cin = cur
        for name, c in zip(["netOne", "netTwo", "netThr", "netFou", "netFiv"], _DENSE):
            setattr(self, name, _seq((cin, c, 1)))
            cin += c
        self.netSix = nn.Sequential(nn.Conv2d(cin, 2, 3, 1, 1))

    def dense(self):
        return [self.netOne, self.netTwo, self.netThr, self.netFou, self.netFiv]


class _Refiner(nn.Module):
    def __init__(self):
        super().__init__()
        self.netMain = _seq((565, 128, 1), (128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16), (64, 32, 1), (32, 2, 1))


class PWCNET(nn.Module):
    """models/pwc_net.py:PWCNET without the weight file read in its constructor (see `load_pwc_weights`).  forward(first,
    second): (N, 3, H, W) each, H and W multiples of 64 -> the flow (N, 2, H/4, W/4) first -> second."""

    def __init__(self):
        super().__init__()
        self.netExtractor = _Extractor()
        self.netTwo = _Decoder(2)
        self.netThr = _Decoder(3)
        self.netFou = _Decoder(4)
        self.netFiv = _Decoder(5)
        self.netSix = _Decoder(6)
        self.netRefiner = _Refiner()

    def forward(self, first: Tensor, second: Tensor) -> Tensor:
        if first.shape != second.shape:
            raise ValueError(f"PWCNET: shapes {tuple(first.shape)} / {tuple(second.shape)} differ")
        n = first.shape[0]
        images = torch.empty((2 * n,) + tuple(first.shape[1:]), device=first.device, dtype=torch.float32)
        images[:n].copy_(first)
        images[n:].copy_(second)
        return self.forward_stacked(images)

    def forward_stacked(self, images: Tensor) -> Tensor:
        """The flow of pair i = (images[i], images[N + i]), i < N = len(images) / 2."""
        if not images.is_cuda:
            raise RuntimeError("PWCNET runs on the GPU only (no CPU path)")
        n2, _, hh, ww = images.shape
        if n2 % 2 or hh % 64 or ww % 64:
            raise ValueError(f"PWCNET: {tuple(images.shape)}: an even number of images of a multiple of 64 px")
        n = n2 // 2
        dev = images.device
        decoders = {2: self.netTwo, 3: self.netThr, 4: self.netFou, 5: self.netFiv, 6: self.netSix}
        # one buffer per decoder level, all 2N rows (the extractor writes every image's features into the `first` slice)
        bufs = {}
        for level in range(2, 7):
            h, w = hh >> level, ww >> level
            bufs[level] = torch.empty((n2, _current(level) + _DENSE_TOP, h, w), device=dev, dtype=torch.float32)
        feats = {}
        x = images
        for level, seq in enumerate(self.netExtractor.levels(), start=1):
            x = ops.pwc_conv3x3(x, seq[0].weight, seq[0].bias, stride=2)
            x = ops.pwc_conv3x3(x, seq[2].weight, seq[2].bias)
            dst = None
            if 2 <= level <= 5:
                off = _DENSE_TOP + 81
                dst = bufs[level][:, off:off + _CH[level - 1]]
            x = ops.pwc_conv3x3(x, seq[4].weight, seq[4].bias, out=dst)
            feats[level] = x
        flow = None
        for level in range(6, 1, -1):
            dec, buf = decoders[level], bufs[level]
            d = buf[:n]
            c = _CH[level - 1]
            vol = d[:, _DENSE_TOP:_DENSE_TOP + 81]
            if level == 6:
                ops.pwc_correlation(feats[6][:n], feats[6][n:], out=vol)
            else:
                off = _DENSE_TOP + 81
                upflow = d[:, off + c:off + c + 2]
                ops.pwc_deconv4x4s2(flow, dec.netUpflow.weight, dec.netUpflow.bias, out=upflow)
                ops.pwc_deconv4x4s2(bufs[level + 1][:n], dec.netUpfeat.weight, dec.netUpfeat.bias, out=d[:, off + c + 2:off + c + 4])
                warped = ops.pwc_backwarp(buf[n:, off:off + c], upflow, dec.fltBackwarp)
                ops.pwc_correlation(d[:, off:off + c], warped, out=vol)
            top = _DENSE_TOP
            for seq, cout in zip(dec.dense(), _DENSE):
                ops.pwc_conv3x3(d[:, top:], seq[0].weight, seq[0].bias, out=d[:, top - cout:top])
                top -= cout
            flow = ops.pwc_conv3x3(d, dec.netSix[0].weight, dec.netSix[0].bias, act=None)
        r = bufs[2][:n]
        main = self.netRefiner.netMain
        for i in range(0, len(main), 2):
            conv = main[i]
            last = i == len(main) - 1
            r = ops.pwc_conv3x3(r, conv.weight, conv.bias, dilation=conv.dilation[0], act=None if last else "lrelu")
        return ops.add(flow, r)


def load_pwc_weights(net: PWCNET, path: str) -> PWCNET:
    """The sniklaus `network-default` file the reference reads (models/pwc_net.py:245-247): its keys say `module` where the
    module tree says `net` (`moduleExtractor.moduleOne.0.weight`); keys already renamed load as they are."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    net.load_state_dict({k.replace("module", "net"): v for k, v in sd.items()}, strict=True)
    return net


def estimate(first: Tensor, second: Tensor, net: PWCNET) -> Tensor:
    """BaseModel.estimate (base_model.py:294-319): the flow first -> second (N, 2, h, w) at the input size, in pixels"""
    if first.shape != second.shape:
        raise ValueError(f"estimate: shapes {tuple(first.shape)} / {tuple(second.shape)} differ")
    n, c, h, w = first.shape
    hp, wp = int(math.ceil(h / 64.0) * 64), int(math.ceil(w / 64.0) * 64)
    images = torch.empty((2 * n, c, hp, wp), device=first.device, dtype=torch.float32)
    ops.resize_bilinear(first, (hp, wp), out=images[:n])
    ops.resize_bilinear(second, (hp, wp), out=images[n:])
    flow = net.forward_stacked(images)
    return ops.resize_bilinear(flow, (h, w), channel_mul=(20.0 * float(w) / float(wp), 20.0 * float(h) / float(hp)))


def get_backwarp(lr: Tensor, hr: Tensor, net: PWCNET, scale: int) -> Tuple[Tensor, Tensor]:
    """BaseModel.get_backwarp (base_model.py:338-354) with flow=None: (hr_align (N, 3, H, W), mask (N, 1, H, W)).  The flow
    LR -> HR downscaled (bilinear, align_corners=True) is read nearest-upsampled x scale and multiplied by scale in place."""
    n, _, h, w = lr.shape
    hh, ww = int(hr.shape[2]), int(hr.shape[3])
    if hh != h * scale or ww != w * scale:
        raise ValueError(f"get_backwarp: HR {hh}x{ww} is not LR {h}x{w} x {scale}")
    with torch.no_grad():
        hr_small = ops.resize_bilinear_ac(hr, (hh // scale, ww // scale))
        flow = estimate(lr, hr_small, net)
        return ops.pwc_backwarp(hr, flow, float(scale), with_mask=True)
