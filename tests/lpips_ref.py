"""LPIPS (AlexNet) restated from its published definition (lpips 0.1, LPIPS(net='alex'), eval mode, spatial=False, normalize=False)
in plain torch on the CPU, for the tests to compare the HIP kernels with.  Written independently of eavsr_amd/lpips.py and never
importing it: plain F.conv2d / F.max_pool2d, in whatever dtype the caller asks for (float64: the reference; float32: the yardstick
of what fp32 arithmetic costs).  Neither the `lpips` package nor torchvision exists where the tests run, so this restatement, not
the package, is what "parity" means in tests/test_hip_lpips.py.

Weights are a plain dict in the package's state-dict layout:
  net.slice1.0 / slice2.3 / slice3.6 / slice4.8 / slice5.10 (.weight, .bias), lin0..4.model.1.weight, scaling_layer.shift / .scale
"""
import math

import torch
import torch.nn.functional as F

# (key prefix, cin, cout, kernel, stride, padding, max-pool in front)
LAYERS = [("net.slice1.0", 3, 64, 11, 4, 2, False), ("net.slice2.3", 64, 192, 5, 1, 2, True), ("net.slice3.6", 192, 384, 3, 1, 1, True),
          ("net.slice4.8", 384, 256, 3, 1, 1, False), ("net.slice5.10", 256, 256, 3, 1, 1, False)]
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def synthetic_weights(seed: int = 0):
    """Trained-like synthetic weights: He-scaled convolutions (features keep an O(1) size through the five layers), small biases
    of both signs (ReLU kills a real share of the activations), non-negative lin weights about a third of which are exactly 0 (the
    trained ones are non-negative and sparse)."""
    g = torch.Generator().manual_seed(4242 + seed)
    sd = {}
    for key, cin, cout, k, _, _, _ in LAYERS:
        fan_in = cin * k * k
        sd[key + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / fan_in)
        sd[key + ".bias"] = (torch.rand(cout, generator=g) - 0.6) * 0.5
    for i, (_, _, cout, _, _, _, _) in enumerate(LAYERS):
        w = torch.rand(1, cout, 1, 1, generator=g)
        w = torch.where(torch.rand(1, cout, 1, 1, generator=g) < 0.35, torch.zeros_like(w), w) * (100.0 / cout)
        sd[f"lin{i}.model.1.weight"] = w
    sd["scaling_layer.shift"] = torch.tensor(SHIFT).view(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(SCALE).view(1, 3, 1, 1)
    return sd


def quantise(v, scale):
    """the 8-bit image of get_current_visuals: round half to even, as torch.round does"""
    return torch.clamp(v * scale, 0, 255).round()


def front_end(v, sd, scale, dtype):
    """steps 1 and 2: fp32 samples -> the scaling layer's output in `dtype`"""
    q = quantise(v.float(), scale).to(dtype)
    x = q / 127.5 - 1.0
    return (x - sd["scaling_layer.shift"].to(dtype)) / sd["scaling_layer.scale"].to(dtype)


def layer(x, sd, index):
    """stage `index` (0..4) of AlexNet.features on x: [max-pool 3/2,] convolution, ReLU; in x's dtype"""
    key, _, _, _, stride, pad, pool = LAYERS[index]
    if pool:
        x = F.max_pool2d(x, 3, 2)
    return F.relu(F.conv2d(x, sd[key + ".weight"].to(x.dtype), sd[key + ".bias"].to(x.dtype), stride=stride, padding=pad))


def tap_distance(fa, fb, lin):
    """step 4 for one tap: (F,) means over the pixels of sum_c lin_c (fa^ - fb^)^2"""
    na = fa / (torch.sqrt(torch.sum(fa * fa, dim=1, keepdim=True)) + 1e-10)
    nb = fb / (torch.sqrt(torch.sum(fb * fb, dim=1, keepdim=True)) + 1e-10)
    d = torch.sum(lin.to(fa.dtype).view(1, -1, 1, 1) * (na - nb) ** 2, dim=1)
    return d.mean(dim=(1, 2))


def features(v, sd, scale=255.0, dtype=torch.float64):
    """the five tapped feature maps of fp32 images v (N, 3, H, W)"""
    h, w = v.shape[-2:]
    if min(h, w) < 31:
        raise ValueError(f"lpips_ref: frame {h} x {w} smaller than 31 pixels on a side")
    x = front_end(v, sd, scale, dtype)
    out = []
    for i in range(5):
        x = layer(x, sd, i)
        out.append(x)
    return out


def lpips(sr, hr, sd, scale=255.0, dtype=torch.float64):
    """per-frame LPIPS of (F, 3, H, W) fp32 tensors, in `dtype`"""
    if sr.shape != hr.shape or sr.dim() != 4 or sr.shape[1] != 3:
        raise ValueError(f"lpips_ref: (F, 3, H, W) tensors of one shape, got {tuple(sr.shape)} / {tuple(hr.shape)}")
    with torch.no_grad():
        fa, fb = features(sr, sd, scale, dtype), features(hr, sd, scale, dtype)
        total = torch.zeros(sr.shape[0], dtype=dtype)
        for i in range(5):
            total = total + tap_distance(fa[i], fb[i], sd[f"lin{i}.model.1.weight"])
        return total


def image_pair(f, h, w, seed=0):
    """(sr, hr) fp32 (F, 3, h, w) in [0, 1]: hr a smooth random texture with some fine detail, sr = hr blurred (two binomial
    passes) plus noise of a few grey levels -- the kind of difference a super-resolution output has, not two independent noises"""
    g = torch.Generator().manual_seed(900 + seed)
    base = torch.rand(f, 3, h // 4 + 3, w // 4 + 3, generator=g)
    hr = F.interpolate(base, scale_factor=4, mode="bicubic", align_corners=False)[:, :, 4:4 + h, 4:4 + w]
    hr = (hr + 0.08 * torch.rand(f, 3, h, w, generator=g)).clamp(0.0, 1.0).contiguous()
    k = torch.tensor([1.0, 2.0, 1.0])
    k2 = (k[:, None] * k[None, :] / 16.0).view(1, 1, 3, 3).repeat(3, 1, 1, 1)
    blur = hr
    for _ in range(2):
        blur = F.conv2d(F.pad(blur, (1, 1, 1, 1), mode="replicate"), k2, groups=3)
    sr = (blur + torch.randn(f, 3, h, w, generator=g) * (4.0 / 255.0)).contiguous()      # not clamped: the kernel clamps
    return sr, hr
