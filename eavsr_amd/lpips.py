"""LPIPS with the AlexNet backbone -- the third column of the reference's score table (psnr_total.py:27-35, :116-138) -- on HIP
kernels (csrc/lpips.hip), so that a checkpoint's evaluation never leaves the GPU.

What is computed is the PUBLISHED definition of `lpips.LPIPS(net='alex')` (lpips 0.1, eval mode, spatial=False, normalize=False)
on the 8-bit images as psnr_total.py reads them back from the PNG files:

  1. q = rint(clamp(v * scale, 0, 255)), half to even (the quantiser of `ops.frame_metrics`); x = q / 127.5 - 1, RGB order;
  2. the scaling layer: (x - shift) / scale per channel, shift = (-.030, -.088, -.188), scale = (.458, .448, .450);
  3. AlexNet `features`, tapped after each ReLU: conv 3->64 11x11 stride 4 pad 2 | maxpool 3/2, conv 64->192 5x5 pad 2 | maxpool
     3/2, conv 192->384 3x3 pad 1 | conv 384->256 3x3 pad 1 | conv 256->256 3x3 pad 1;
  4. per tap and pixel f^ = f / (sqrt(sum_c f^2) + 1e-10), d = sum_c w_c (f^_sr - f^_hr)^2 with the tap's 1x1 `lin` weight, the
     tap's mean of d over its pixels; LPIPS = the sum of the five means.

Neither the `lpips` package nor torchvision is a dependency, and no pretrained weights ship with this project: the network is built
here and its weights come from a path the user names (`opt.lpips_path`), as PWC-Net's do.  The metric is therefore pinned to the
definition above, not to the package: the tests compare with a float64 restatement of these four steps on synthetic weights
(tests/lpips_ref.py), never with the package's output.  The state-dict key tables below are written from the published packages'
module trees (lpips 0.1 `LPIPS`, torchvision `AlexNet`), not from weight files: nobody here has loaded a real `alex.pth` yet.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import ops

Tensor = torch.Tensor

# (slice name, index of the convolution in torchvision's AlexNet.features, cin, cout, kernel, stride, padding)
_CONVS = [("slice1", 0, 3, 64, 11, 4, 2), ("slice2", 3, 64, 192, 5, 1, 2), ("slice3", 6, 192, 384, 3, 1, 1),
          ("slice4", 8, 384, 256, 3, 1, 1), ("slice5", 10, 256, 256, 3, 1, 1)]
MIN_SIDE = 31      # smaller frames leave no pixel after the second max-pool


class _Slices(nn.Module):
    """lpips' `alexnet` wrapper: five nn.Sequential slices whose children keep torchvision's `features` indices"""

    def __init__(self):
        super().__init__()
        for name, idx, cin, cout, k, s, p in _CONVS:
            seq = nn.Sequential()
            seq.add_module(str(idx), nn.Conv2d(cin, cout, k, s, p))
            setattr(self, name, seq)


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.tensor([.458, .448, .450])[None, :, None, None])


class _NetLinLayer(nn.Module):
    """lpips' NetLinLayer: [Dropout, Conv2d(C, 1, 1, bias=False)]; only the convolution (child 1) has state"""

    def __init__(self, cin: int):
        super().__init__()
        self.model = nn.Sequential(nn.Identity(), nn.Conv2d(cin, 1, 1, bias=False))


class LPIPSAlex(nn.Module):
    """`lpips.LPIPS(net='alex')` with the package's state-dict keys (`net.slice1.0.weight` ... `net.slice5.10.bias`,
    `lin0.model.1.weight` ... `lin4.model.1.weight`, buffers `scaling_layer.shift` / `scaling_layer.scale`), frozen, forward on the
    eavsr_lpips_* entry points only.  The parameters are freshly initialised until `load_lpips_weights` fills them."""

    def __init__(self):
        super().__init__()
        self.scaling_layer = _ScalingLayer()
        self.net = _Slices()
        for k, (_, _, _, cout, _, _, _) in enumerate(_CONVS):
            setattr(self, f"lin{k}", _NetLinLayer(cout))
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()

    def convs(self):
        return [getattr(self.net, name)[0] for name, *_ in _CONVS]

    def lins(self):
        return [getattr(self, f"lin{k}").model[1] for k in range(5)]

    def features(self, sr: Tensor, hr: Tensor, scale: float = 255.0):
        """the five tapped feature maps of the batch [sr frames, hr frames]: (2F, C_k, h_k, w_k) each"""
        c = self.convs()
        sl = self.scaling_layer
        f1 = ops.lpips_conv1(sr, hr, c[0].weight, c[0].bias, sl.shift, sl.scale, scale)
        f2 = ops.lpips_conv(ops.lpips_maxpool(f1), c[1].weight, c[1].bias)
        f3 = ops.lpips_conv(ops.lpips_maxpool(f2), c[2].weight, c[2].bias)
        f4 = ops.lpips_conv(f3, c[3].weight, c[3].bias)
        f5 = ops.lpips_conv(f4, c[4].weight, c[4].bias)
        return [f1, f2, f3, f4, f5]

    @torch.no_grad()
    def forward(self, sr: Tensor, hr: Tensor, scale: float = 255.0) -> Tensor:
        """sr, hr (F, 3, H, W) or (n, t, 3, H, W) device tensors (scale 255: [0, 1] tensors; scale 1: `get_current_visuals()`
        tensors) -> float64 per-frame LPIPS, (F,) or (n, t).  H, W >= 31."""
        if not isinstance(sr, torch.Tensor) or not isinstance(hr, torch.Tensor):
            raise TypeError("LPIPSAlex: tensors expected")
        if not sr.is_cuda or not hr.is_cuda:
            raise RuntimeError("LPIPSAlex runs on the GPU only (no CPU path)")
        if sr.shape != hr.shape or sr.dim() not in (4, 5) or sr.shape[-3] != 3:
            raise ValueError(f"LPIPSAlex: (F, 3, H, W) or (n, t, 3, H, W) tensors of one shape, got {tuple(sr.shape)} / {tuple(hr.shape)}")
        h, w = int(sr.shape[-2]), int(sr.shape[-1])
        if min(h, w) < MIN_SIDE:
            raise ValueError(f"LPIPSAlex: frame {h} x {w} smaller than {MIN_SIDE} pixels on a side: no pixel is left after the second "
                             "max-pool")
        lead = tuple(sr.shape[:-3])
        sr = sr.detach().reshape(-1, 3, h, w).contiguous()
        hr = hr.detach().reshape(-1, 3, h, w).contiguous()
        out = None
        for feat, lin in zip(self.features(sr, hr, scale), self.lins()):
            out = ops.lpips_tap(feat, lin.weight, out=out)
        return out.view(lead)


def _expected_shapes(net: LPIPSAlex) -> Dict[str, tuple]:
    return {k: tuple(v.shape) for k, v in net.state_dict().items()}


def _read(path: str) -> Dict[str, Tensor]:
    if not os.path.isfile(path):
        raise FileNotFoundError(f"LPIPS weights {path!r} not found")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise RuntimeError(f"{path}: not a state dict")
    return sd


def _is_lins_alias(key: str) -> bool:
    """`lins.k.model.1.weight`: the package registers the five lin layers a second time in an nn.ModuleList"""
    parts = key.split(".")
    return len(parts) == 5 and parts[0] == "lins" and parts[1].isdigit() and parts[2:] == ["model", "1", "weight"]


def load_lpips_weights(net: LPIPSAlex, path: str, alexnet_path: Optional[str] = None) -> LPIPSAlex:
    """Fill `net` from either layout, with the strictness of `load_networks` (an unknown key, a missing key or a wrong shape raises
    and names the key):
      * `path` alone: one file holding the module's own state dict (`lpips.LPIPS(net='alex').state_dict()`); the package's
        `lins.k.model.1.weight` aliases of `link.model.1.weight` are accepted and ignored;
      * `path` + `alexnet_path`: the pair the packages distribute -- the lpips `alex.pth` (`lin{k}.model.1.weight` only) and a
        torchvision AlexNet state dict (`features.{0,3,6,8,10}.{weight,bias}`; `classifier.*` ignored).  The scaling layer's
        buffers keep their published constants.
    Several processes: every rank reads its files and the ranks agree (`shard.all_ranks_ok`) before any of them goes on."""
    from .shard import all_ranks_ok
    err = None
    try:
        own = _expected_shapes(net)
        sd = {k: v for k, v in _read(path).items() if not _is_lins_alias(k)}
        if alexnet_path is not None:
            for k in sd:
                if not (k.startswith("lin") and k in own):
                    raise RuntimeError(f"{path}: unexpected key [{k}] (the lin file holds lin0..4.model.1.weight only)")
            feats = _read(alexnet_path)
            index_to_slice = {idx: name for name, idx, *_ in _CONVS}
            for k, v in feats.items():
                if k.startswith("classifier."):
                    continue
                parts = k.split(".")
                if len(parts) != 3 or parts[0] != "features" or not parts[1].isdigit() or int(parts[1]) not in index_to_slice \
                        or parts[2] not in ("weight", "bias"):
                    raise RuntimeError(f"{alexnet_path}: unexpected key [{k}] (torchvision AlexNet: features.{{0,3,6,8,10}}.*)")
                sd[f"net.{index_to_slice[int(parts[1])]}.{parts[1]}.{parts[2]}"] = v
            for k in ("scaling_layer.shift", "scaling_layer.scale"):
                sd[k] = net.state_dict()[k]
        where = path if alexnet_path is None else f"{path} + {alexnet_path}"
        for k in sd:
            if k not in own:
                raise RuntimeError(f"{where}: unexpected key [{k}] is not a parameter of LPIPSAlex")
        for k in own:
            if k not in sd:
                raise RuntimeError(f"Parameter named [{k}] is not in {where}")
        for k, v in sd.items():
            if not isinstance(v, torch.Tensor) or tuple(v.shape) != own[k]:
                raise RuntimeError(f"While copying the parameter named [{k}], whose dimensions in the model are {list(own[k])} and "
                                   f"whose dimensions in the checkpoint are {list(getattr(v, 'shape', ()))}.")
        net.load_state_dict({k: v.to(torch.float32) for k, v in sd.items()}, strict=True)
    except Exception as e:      # noqa: BLE001 -- re-raised below, on every rank
        err = e
    if not all_ranks_ok(err is None):
        if err is not None:
            raise err
        raise RuntimeError("another rank failed to load the LPIPS weights; aborting on every rank")
    return net


def build_lpips(path: str, alexnet_path: Optional[str] = None, device=None) -> LPIPSAlex:
    """An `LPIPSAlex` with the weights of `path` (see `load_lpips_weights`) on `device`, frozen, in eval mode"""
    net = load_lpips_weights(LPIPSAlex(), path, alexnet_path)
    if device is not None:
        net = net.to(device)
    return net.eval()
