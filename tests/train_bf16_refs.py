"""float64 references of the bf16 training mode's kernels (tests/test_hip_train_bf16.py; checked on the CPU by
tests/test_train_precision_host.py).  Operands are rounded to bf16 ONCE, by torch (nearest even) or by truncation (what the
mode must not do); the convolution of the rounded values is then exact in float64, and S = sum |a| |b| over the same terms
bounds what fp32 accumulation may add to it."""
import torch


def bf16_rne(t):
    """t rounded to bf16, nearest even, as float64"""
    return t.to(torch.bfloat16).to(torch.float64)


def bf16_trunc(t):
    """t truncated to bf16 (the upper 16 bits of its fp32 pattern), as float64"""
    u = t.to(torch.float32).contiguous().view(torch.int32) & ~0xFFFF
    return u.view(torch.float32).to(torch.float64)


def conv3x3_ref(x, w, bias=None):
    """float64 stride-1 'same' 3x3 convolution of x (n, cin, h, w) with w (cout, cin, 3, 3), and S = the same convolution of |x|
    and |w| (the bound's scale)"""
    x, w = x.to(torch.float64), w.to(torch.float64)
    y = torch.nn.functional.conv2d(x, w, None if bias is None else bias.to(torch.float64), padding=1)
    s = torch.nn.functional.conv2d(x.abs(), w.abs(), None, padding=1)
    return y, s


def wgrad3x3_ref(dys, xs):
    """float64 weight gradient sum_seg sum_{n,y,x} dy[n,co,y,x] x[n,ci,y+ky-1,x+kx-1] over the segments (lists of tensors), and S
    = the same of |dy| and |x|"""
    g = s = None
    for dy, x in zip(dys, xs):
        dy, x = dy.to(torch.float64), x.to(torch.float64)
        gi = torch.nn.grad.conv2d_weight(x, (dy.shape[1], x.shape[1], 3, 3), dy, padding=1)
        si = torch.nn.grad.conv2d_weight(x.abs(), (dy.shape[1], x.shape[1], 3, 3), dy.abs(), padding=1)
        g, s = (gi, si) if g is None else (g + gi, s + si)
    return g, s
