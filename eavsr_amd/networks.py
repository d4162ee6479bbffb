"""Drop-in counterparts of the hot-path classes of the reference's models/networks.py.

Same class names, constructor arguments, forward() signatures and state_dict keys as the
reference (so `load_networks`, which exits on any key mismatch -- base_model.py:193-213 -- keeps
working), but every forward() runs hand-written HIP kernels from libeavsr_hip.so through
eavsr_amd.ops.  The modules can be *constructed* and (de)serialised on any device; calling them
needs fp32 tensors on a MI355X -- there is no CPU or PyTorch-op fallback.

Only what EAVSRP instantiates is here (rows 2-6, 8); the dead classes of
networks.py (PatchSelect, ResBlock*, Flownet, SPYAdaSTN, ...) are out of scope.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import List, Sequence, Union

import torch
import torch.nn as nn

from . import autograd as AG
from . import ops

Tensor = torch.Tensor
TensorOrList = Union[Tensor, Sequence[Tensor]]


# --------------------------------------------------------------------------------------------
# layer-string builder (networks.py:84-95 `seq`, :108-190 `conv`): only the modes the hot path uses
# --------------------------------------------------------------------------------------------
def seq(*args):
    if len(args) == 1:
        args = args[0]
    if isinstance(args, nn.Module):
        return args
    return nn.Sequential(*[seq(a) for a in args])


class Conv2d(nn.Conv2d):
    """nn.Conv2d parameter container (same keys / default init) whose forward is the MFMA conv.
    Dense stride-1 "same" convolutions only; `act` fuses the activation that follows it in the
    reference's nn.Sequential."""

    def forward(self, x: TensorOrList, act=None, slope=0.0, residual=None, chan_partial=False, pixel_shuffle2=False):
        if self.groups != 1 or self.stride != (1, 1) or self.dilation != (1, 1) or \
                self.padding != (self.kernel_size[0] // 2,) * 2 or self.padding_mode != "zeros":
            raise NotImplementedError("eavsr_amd Conv2d: dense stride-1 same-padding convolutions only")
        return AG.conv2d(x, self.weight, self.bias, act=act, slope=slope, residual=residual,
                         chan_partial=chan_partial, pixel_shuffle2=pixel_shuffle2)


class _Act(nn.Module):
    """Placeholder that keeps nn.Sequential indices (hence state_dict keys) identical to the
    reference; the activation itself is fused into the preceding conv's epilogue."""

    def __init__(self, kind: str, slope: float = 0.0):
        super().__init__()
        self.kind, self.slope = kind, slope

    def extra_repr(self):
        return f"{self.kind}, slope={self.slope} (fused)"


def conv(in_channels=64, out_channels=64, kernel_size=3, stride=1, padding=1, bias=True, groups=1, mode="CBR"):
    """networks.py:108-190 for the modes EAVSRP uses: 'C', 'R', 'L' (LeakyReLU 0.2)."""
    L = []
    for t in mode:
        if t == "C":
            L.append(Conv2d(in_channels, out_channels, kernel_size, stride, padding, groups=groups, bias=bias))
        elif t in "Rr":
            L.append(_Act("relu"))
        elif t in "Ll":
            L.append(_Act("lrelu", 0.2))
        else:
            raise NotImplementedError(f"conv mode {t!r} is not used on the EAVSR hot path")
    return seq(*L)


def _run_fused(seq_mod: nn.Sequential, x: TensorOrList, residual=None, chan_partial=False):
    """Run a Sequential of Conv2d / _Act with each activation fused into the conv before it."""
    mods = list(seq_mod) if isinstance(seq_mod, nn.Sequential) else [seq_mod]
    i, out = 0, x
    while i < len(mods):
        m = mods[i]
        if not isinstance(m, Conv2d):
            raise NotImplementedError(type(m))
        act, slope = None, 0.0
        if i + 1 < len(mods) and isinstance(mods[i + 1], _Act):
            act, slope = mods[i + 1].kind, mods[i + 1].slope
            i += 1
        last = i == len(mods) - 1
        out = m(out, act=act, slope=slope, residual=residual if last else None,
                chan_partial=chan_partial and last)
        i += 1
    return out


# --------------------------------------------------------------------------------------------
# flow_warp  (networks.py:699-739)
# --------------------------------------------------------------------------------------------
def flow_warp(x, flow, interpolation="bilinear", padding_mode="zeros", align_corners=True):
    """Warp `x` (n,c,h,w) by `flow` (n,2,h,w; channel 0 = x displacement, 1 = y, in pixels)."""
    return AG.flow_warp(x, flow, padding_mode=padding_mode, flow_layout="nchw", interpolation=interpolation,
                        align_corners=align_corners)


# --------------------------------------------------------------------------------------------
# DCNv2 (mmcv.ops stand-ins: networks.py:573)
# --------------------------------------------------------------------------------------------
modulated_deform_conv2d = AG.modulated_deform_conv2d


class ModulatedDeformConv2d(nn.Module):
    """Parameter-compatible with mmcv.ops.ModulatedDeformConv2d (weight, bias; mmcv's default init
    uniform(+-1/sqrt(cin*kh*kw)), zero bias)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deform_groups=1, bias=True):
        super().__init__()
        ks = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, ks
        self.stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
        self.padding = (padding, padding) if isinstance(padding, int) else tuple(padding)
        self.dilation = (dilation, dilation) if isinstance(dilation, int) else tuple(dilation)
        self.groups, self.deform_groups = groups, deform_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *ks))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.init_weights()

    def init_weights(self):
        n = self.in_channels
        for k in self.kernel_size:
            n *= k
        stdv = 1.0 / math.sqrt(n)
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.zero_()

    def forward(self, x, offset, mask):
        return modulated_deform_conv2d(x, offset, mask, self.weight, self.bias, self.stride, self.padding,
                                       self.dilation, self.groups, self.deform_groups)


# --------------------------------------------------------------------------------------------
# offset predictors (networks.py:280-348, 566-571)
# --------------------------------------------------------------------------------------------
_REGULAR = [[-1, -1, -1, 0, 0, 0, 1, 1, 1], [-1, 0, 1, -1, 0, 1, -1, 0, 1]]


class _AdaptBase(nn.Module):
    def __init__(self, inplanes):
        super().__init__()
        self.register_buffer("regular_matrix", torch.tensor(_REGULAR).float())
        self.concat = conv(inplanes * 2, inplanes * 2, groups=inplanes * 2, mode="CL")
        self.concat2 = conv(inplanes * 2, inplanes, groups=inplanes, mode="CL")

    def _frontend(self, x, h_hr, out=None):
        """out (inference only): rows of a frame-major stack to write into"""
        c1, c2 = self.concat[0], self.concat2[0]
        if out is not None:
            return ops.adapt_frontend(x, h_hr, c1.weight, c1.bias, c2.weight, c2.bias, out=out)
        return AG.adapt_frontend(x, h_hr, c1.weight, c1.bias, c2.weight, c2.bias)


class AdaptBlock2_3x3(_AdaptBase):
    """networks.py:318-348: (x, h_hr) -> 18 sampling offsets of one 3x3 grid."""

    def __init__(self, opt, inplanes=64, outplanes=64, stride=1, dilation=1, deformable_groups=64):
        super().__init__(inplanes)
        self.opt = opt
        self.mask = True
        self.transform_matrix_conv = Conv2d(inplanes, 4, 3, 1, 1, bias=True)
        self.translation_conv = Conv2d(inplanes, 2, 3, 1, 1, bias=True)

    def forward(self, x, h_hr):
        f = self._frontend(x, h_hr)
        heads = AG.conv2d(f, [self.transform_matrix_conv.weight, self.translation_conv.weight],
                          [self.transform_matrix_conv.bias, self.translation_conv.bias])
        return AG.affine_offsets(heads, 1, with_mask=False)[0]


class AdaptBlockOffset(_AdaptBase):
    """networks.py:280-315: (x, h_hr) -> (offset (n,18D,h,w) in mmcv order, mask (n,9D,h,w))."""

    def __init__(self, opt, inplanes=64, outplanes=64, stride=1, dilation=1, deformable_groups=64):
        super().__init__(inplanes)
        self.D = deformable_groups
        self.opt = opt
        self.transform_matrix_conv = Conv2d(inplanes, 4 * self.D, 5, 1, 2, bias=True)
        self.translation_conv = Conv2d(inplanes, 2 * self.D, 5, 1, 2, bias=True)
        self.mask_conv = Conv2d(inplanes, 9 * self.D, 5, 1, 2, bias=True)
        self.relu = _Act("lrelu", 0.2)  # unused by forward in the reference as well

    def heads(self, x, h_hr, mask_activated=False):
        """the three 5x5 heads as one (n, 15 D, h, w) tensor: transform g*4+{0..3}, translation 4D + g*2+{0,1}, mask logits
        6D + g*9+k -- what `forward` expands into (offset, mask) and what the fused DCNv2 kernel consumes directly.
        mask_activated: the 9 D mask channels leave as sigmoid(logit) (networks.py:313-314 applied in the convolution's epilogue)"""
        return self.heads_of(self._frontend(x, h_hr), mask_activated)

    def heads_of(self, f, mask_activated=False):
        """`heads` behind the front end: the 5x5 convolutions on its output f (n, 64, h, w) -- any number of images in one launch"""
        ws = [self.transform_matrix_conv.weight, self.translation_conv.weight, self.mask_conv.weight]
        bs = [self.transform_matrix_conv.bias, self.translation_conv.bias, self.mask_conv.bias]
        if (BACKBONE_DTYPE is not None and HEADS_IN_16BIT and f.shape[1] == 64 and 15 * self.D <= 128
                and not AG.needs_grad(f, ws, bs)):
            # 16-bit modes (BASELINE configs[2] / [4]): operands rounded once to bf16 / fp16, fp32 accumulation, fp32 heads out
            return ops.conv5x5_c64_h16(ops.to_nhwc_h16(f, BACKBONE_DTYPE), ws, bs)
        if mask_activated:
            return ops.conv2d(f, ws, bs, sigmoid_from=6 * self.D)
        return AG.conv2d(f, ws, bs)

    def forward(self, x, h_hr):
        return AG.affine_offsets(self.heads(x, h_hr), self.D, with_mask=True)


class TransOffsetworelu(nn.Module):
    """networks.py:566-571: 3x3 conv 18 -> 2 ("offsets -> residual flow"), no activation."""

    def __init__(self):
        super().__init__()
        self.conv_first = conv(18, 2, mode="C")

    def forward(self, offset):
        return self.conv_first(offset)


class MultiAdSTN(ModulatedDeformConv2d):
    """networks.py:575-631.  forward(nbr_feat_l, ref_feat_l, feat_prop, offset, flag=False)."""

    def __init__(self, opt, inplanes=64, outplanes=64, stride=1, dilation=1, deformable_groups=64):
        super().__init__(inplanes, outplanes, kernel_size=3, padding=1, stride=stride, dilation=dilation,
                         deform_groups=deformable_groups)
        self.opt = opt
        kw = dict(inplanes=inplanes, outplanes=outplanes, stride=stride, dilation=dilation,
                  deformable_groups=deformable_groups)
        self.flow_l1 = AdaptBlock2_3x3(opt, **kw)
        self.flow_l2 = AdaptBlock2_3x3(opt, **kw)
        self.flow_l3 = AdaptBlock2_3x3(opt, **kw)
        self.adastn = AdaptBlockOffset(opt, **kw)
        self.trans_l3 = TransOffsetworelu()
        self.trans_l2 = TransOffsetworelu()
        self.trans_l1 = TransOffsetworelu()
        self.center = getattr(opt, "n_frame", 7) // 2

    @staticmethod
    def _level(flow_blk, trans_blk, warp, ref):
        """trans(flow(warp, ref)): one pyramid level's residual flow (networks.py:605-607 etc.).  Inference: ONE kernel
        (front end, 64 -> 4 + 2 heads, affine -> 18 offsets, 18 -> 2 conv, nothing but the two inputs and the 2-channel flow
        touch HBM); with gradients: the un-fused ops, each with its backward kernel."""
        tconv = trans_blk.conv_first[0] if isinstance(trans_blk.conv_first, nn.Sequential) else trans_blk.conv_first
        params = [warp, ref] + list(flow_blk.parameters()) + list(trans_blk.parameters())
        if FUSE_FLOW_LEVEL and not AG.needs_grad(params) and warp.shape[1] % 2 == 0:
            c1, c2 = flow_blk.concat[0], flow_blk.concat2[0]
            return ops.flow_level(warp, ref, c1.weight, c1.bias, c2.weight, c2.bias,
                                  [flow_blk.transform_matrix_conv.weight, flow_blk.translation_conv.weight],
                                  [flow_blk.transform_matrix_conv.bias, flow_blk.translation_conv.bias],
                                  tconv.weight, tconv.bias)
        return trans_blk(flow_blk(warp, ref))

    def _fused_alignment(self, nbr, feat_prop, offset) -> bool:
        return (ops.DCN_MODE in ("il6", "il9") and not AG.needs_grad(nbr, feat_prop, offset, list(self.parameters()))
                and self.kernel_size == (3, 3) and self.stride == (1, 1) and self.padding == (1, 1)
                and self.dilation == (1, 1) and self.groups == 1 and self.in_channels % 8 == 0
                and (self.in_channels // self.deform_groups) % 8 == 0 and self.adastn.D == self.deform_groups
                and ((self.in_channels // self.deform_groups) // 8) & ((self.in_channels // self.deform_groups) // 8 - 1) == 0
                and nbr.shape == feat_prop.shape)

    def refine(self, nbr_feat_l, ref_feat_l, offset):
        """the three-level residual-flow refinement (networks.py:598-619): flow (n,2,h,w) -> refined offset.  Reads the encoder
        pyramids and the flow only -- nothing of the recurrence."""
        n, _, h, w = offset.shape
        h4, w4 = int(math.floor(h * 0.25)), int(math.floor(w * 0.25))
        h2, w2 = int(math.floor(h * 0.5)), int(math.floor(w * 0.5))
        off_d4 = AG.resize_bilinear_ac(offset, (h4, w4), 0.25)            # :600
        off_d2 = AG.resize_bilinear_ac(offset, (h2, w2), 0.5)             # :601
        # level 3 (:604-608)
        warp4 = AG.flow_warp(nbr_feat_l[2], off_d4)
        p1 = self._level(self.flow_l3, self.trans_l3, warp4, ref_feat_l[2])
        p1_up = AG.resize_bilinear_ac(p1, (2 * h4, 2 * w4), 2.0)
        # level 2 (:609-613)
        warp2 = AG.flow_warp(nbr_feat_l[1], off_d2, flow2=p1_up)
        p2 = self._level(self.flow_l2, self.trans_l2, warp2, ref_feat_l[1])
        p2_up = AG.resize_bilinear_ac(p2, (2 * h2, 2 * w2), 2.0, pre_add=p1_up)
        # level 1 (:614-619)
        warp1 = AG.flow_warp(nbr_feat_l[0], offset, flow2=p2_up)
        p3 = self._level(self.flow_l1, self.trans_l1, warp1, ref_feat_l[0])
        return AG.add(p3, p2_up, offset)

    # -- the module in two halves (inference, fp32 hot path): everything up to the predictor's heads reads per-frame inputs only
    # (encoder pyramids, SPyNet's flow, this module's weights) and can run for ALL time steps of a branch before the first one;
    # the recurrent state enters with the warp of feat_prop and the DCNv2 alone (networks.py:623, :627-630).  The two halves run
    # the launches of `forward`'s fused branch, minus the pair launch's first half, on more images: the same bits.
    def can_split(self, nbr, offset) -> bool:
        """`predict` / `sample` apply: the fused fp32 alignment of `forward` (see _fused_alignment), no gradients anywhere"""
        return BACKBONE_DTYPE is None and self._fused_alignment(nbr, nbr, offset)

    def predict_front(self, nbr_feat_l, ref_feat_l, flow, out=None):
        """(refined offset, the predictor front end's output) of any number of images; `out`: rows of a stack for the latter"""
        offset = self.refine(nbr_feat_l, ref_feat_l, flow)
        nbr = ops.flow_warp_single(nbr_feat_l[0], offset)                                        # :621
        return offset, self.adastn._frontend(nbr, ref_feat_l[0], out=out)                        # :625 (first half)

    def heads_of(self, f):
        """the 15 D head channels of front-end outputs f, the masks activated where `sample`'s kernel takes them so"""
        return self.adastn.heads_of(f, mask_activated=ops.heads_mask_activated(int(self.weight.shape[1]), self.deform_groups))

    def predict(self, nbr_feat_l, ref_feat_l, flow):
        """what `sample` needs beside the recurrent state: (refined offset (n,2,h,w), heads (n,15 D,h,w))"""
        offset, f = self.predict_front(nbr_feat_l, ref_feat_l, flow)
        return offset, self.heads_of(f)

    def sample(self, feat_prop, offset, heads):
        """the recurrent half: ONE warp of feat_prop, written in the IL8 layout, and the heads-mode DCNv2 (:623, :627-630)"""
        feat_il = ops.flow_warp_single(feat_prop, offset, il8=True)
        act = ops.heads_mask_activated(int(self.weight.shape[1]), self.deform_groups)
        return ops.dcnv2_il(feat_il, heads, None, self.weight, self.bias, self.deform_groups,
                            nprod=int(ops.DCN_MODE[2]), heads=True, mask_activated=act)

    def forward(self, nbr_feat_l, ref_feat_l, feat_prop, offset, flag=False):
        if not flag:
            offset = self.refine(nbr_feat_l, ref_feat_l, offset)
        if self._fused_alignment(nbr_feat_l[0], feat_prop, offset):
            # inference hot path: both warps by the refined offset in ONE launch, the second one written in the IL8 layout the
            # DCNv2 kernel samples from; the predictor's 15 D head channels go to that kernel as they are (affine -> offsets
            # and the mask sigmoid, networks.py:302-315, happen in its per-group set-up): de_offset / mask never reach HBM
            if BACKBONE_DTYPE is not None:
                # 16-bit mode (configs[2] / [4]): the warp rounds the sampled features once to bf16 / fp16 (IL8), DCNv2 runs
                # on the 16-bit MFMA with fp32 blend and accumulation; offsets, masks, output stay fp32
                nbr, feat_il = ops.flow_warp_pair(nbr_feat_l[0], feat_prop, offset, b_il8=BACKBONE_DTYPE)
                heads = self.adastn.heads(nbr, ref_feat_l[0])
                return ops.dcnv2_il16(feat_il, heads, None, self.weight, self.bias, self.deform_groups, heads=True)
            nbr, feat_il = ops.flow_warp_pair(nbr_feat_l[0], feat_prop, offset, b_il8=True)          # :621, :623
            act = ops.heads_mask_activated(int(self.weight.shape[1]), self.deform_groups)      # the mask sigmoid in the heads' epilogue (:313-314)
            heads = self.adastn.heads(nbr, ref_feat_l[0], mask_activated=act)                        # :625
            return ops.dcnv2_il(feat_il, heads, None, self.weight, self.bias, self.deform_groups,
                                nprod=int(ops.DCN_MODE[2]), heads=True, mask_activated=act)          # :627-630
        nbr = AG.flow_warp(nbr_feat_l[0], offset)                             # :621
        feat = AG.flow_warp(feat_prop, offset)                                # :623
        de_offset, mask = self.adastn(nbr, ref_feat_l[0])                      # :625
        return modulated_deform_conv2d(feat, de_offset, mask, self.weight, self.bias, self.stride, self.padding,
                                       self.dilation, self.groups, self.deform_groups)   # :627-630


# --------------------------------------------------------------------------------------------
# residual channel-attention backbone (networks.py:432-482)
# --------------------------------------------------------------------------------------------
class CALayer(nn.Module):
    def __init__(self, channel=64, reduction=16):
        super().__init__()
        self.conv_du = nn.Sequential(
            nn.Conv2d(channel, channel // reduction, 1, padding=0, bias=True), _Act("relu"),
            nn.Conv2d(channel // reduction, channel, 1, padding=0, bias=True), _Act("sigmoid"))

    def scale_from_partial(self, partial: Tensor, hw: int) -> Tensor:
        a, b = self.conv_du[0], self.conv_du[2]
        return ops.ca_scale(partial, hw, a.weight, a.bias, b.weight, b.bias)

    def forward(self, x):
        """x * sigmoid(MLP(mean_hw(x))).  Stand-alone form (RCABlock uses the fused path where the
        channel sums come out of the conv epilogue)."""
        n, c, h, w = x.shape
        a, b = self.conv_du[0], self.conv_du[2]
        if AG.needs_grad(x, a.weight, b.weight):
            return AG.rcab_tail(x, torch.zeros_like(x), a.weight, a.bias, b.weight, b.bias)
        partial = x.sum(dim=(2, 3)).view(n, 1, c)
        return ops.scale_residual(x, self.scale_from_partial(partial, h * w), torch.zeros_like(x))


class RCABlock(nn.Module):
    def __init__(self, in_channels=64, out_channels=64, kernel_size=3, stride=1, padding=1, bias=True,
                 mode="CRC", reduction=16):
        super().__init__()
        assert in_channels == out_channels
        if mode[0] in "RL":
            mode = mode[0].lower() + mode[1:]
        self.res = conv(in_channels, out_channels, kernel_size, stride, padding, bias=bias, mode=mode)
        self.ca = CALayer(out_channels, reduction)

    def forward(self, x):
        a, b = self.ca.conv_du[0], self.ca.conv_du[2]
        if AG.needs_grad(x, list(self.parameters())):
            # training: the whole block as one autograd node where it applies (autograd.rcab), else per-op nodes: un-fused mean /
            # MLP / scale so that every piece has its backward kernel
            if (RCAB_ONE_NODE and len(self.res) == 3 and isinstance(self.res[1], _Act) and self.res[1].kind == "relu"
                    and torch.is_grad_enabled()):
                c1, c2 = self.res[0], self.res[2]
                ps = [c1.weight, c1.bias, c2.weight, c2.bias, a.weight, a.bias, b.weight, b.bias]
                if AG.rcab_supported(x, ps):
                    return AG.rcab(x, *ps)
            r = _run_fused(self.res, x)
            return AG.rcab_tail(r, x, a.weight, a.bias, b.weight, b.bias)
        if (RCAB_PRE and x.shape[1] == 64 and len(self.res) == 3 and isinstance(self.res[1], _Act) and self.res[1].kind == "relu"
                and tuple(self.res[2].weight.shape) == (64, 64, 3, 3) and int(a.weight.shape[0]) <= 8):
            # the attention BEFORE the second convolution (ops.ca_scale_pre: its output's channel means are linear in border-corrected
            # channel sums of its input), `res * y + x` as that convolution's epilogue: no scale_residual launch (88 MB of HBM traffic
            # per block at 2 x 64 x 180 x 320)
            c1, c2 = self.res[0], self.res[2]
            # (this branch is inference-only: AG.needs_grad was checked above; the border pieces are a by-product of the first
            # convolution's epilogue where the grouped F(4x4,3x3) kernel runs, None elsewhere: then ca_scale_pre sums the lines itself)
            t, tpart, pieces = ops.conv2d(x, c1.weight, c1.bias, act="relu", chan_partial=True, border=True)
            if not RCAB_PRE_PIECES:
                pieces = None
            scale = ops.ca_scale_pre(t, tpart, c2.weight, c2.bias, a.weight, a.bias, b.weight, b.bias, border=pieces)
            return ops.conv2d(t, c2.weight, c2.bias, residual=x, res_scale=scale)
        r, partial = _run_fused(self.res, x, chan_partial=True)     # conv-ReLU-conv, + channel sums
        if FUSE_CA_TAIL:
            return ops.ca_tail(r, partial, a.weight, a.bias, b.weight, b.bias, x)      # CALayer + res * y + x in one launch
        scale = self.ca.scale_from_partial(partial, x.shape[2] * x.shape[3])
        return ops.scale_residual(r, scale, x)                      # res * y + x  (:463-464)


# Fold `res * y + x` of block k into the first conv of block k+1 (the ca_* fields of the conv descriptor; applied in the
# input transform of the Winograd kernels, in the patch prologue of the direct kernel).  Measured at 4x64x180x320 on the
# F(4x4,3x3) kernel: the fused conv costs +21 us (two input patches, the scale FMA on the transform's critical path, the
# side output) against the 27 us scale_residual launch it removes - 314 ms vs 311 ms per step - so it is off by default.
import os as _os
# The RCAB tail (mean -> MLP -> sigmoid -> res * y + x, networks.py:444-447,463-464) as ONE launch (eavsr_ca_tail_f32) instead of
# ca_scale + scale_residual: EAVSR_FUSE_CA_TAIL=1.  OFF by default.  Round 3's kernel is shaped to run beside a resident
# convolution workgroup (256 threads, 27 registers, 4.6 KB of LDS), is bit-identical and 7.6 us shorter back to back (22.3 against
# 29.9 us per block) -- and the two-stream step is still SLOWER with it, 241.6 -> 249.8 ms (A/B on one box): three 16-register
# scale_residual waves fit per SIMD beside a convolution but one 32-register wave of the fused kernel, each holding its slot through a
# latency-bound MLP prologue, while ca_scale's two workgroups leave the GPU to the other stream.
FUSE_CA_TAIL = _os.environ.get("EAVSR_FUSE_CA_TAIL", "0") == "1"
# fp32 inference: the RCAB's attention before its second convolution, the tail as that convolution's epilogue (as RCAB_H16_PRE in the
# 16-bit modes): 217.0 / 218.0 -> 213.0 / 214.0 ms per configs[1] step in rotation on one box (tools/visits/r5_o.sh), timed output
# bit-identical to the eager forward.  EAVSR_RCAB_PRE=0 keeps conv, conv, ca_scale, scale_residual (A/B switch).
RCAB_PRE = _os.environ.get("EAVSR_RCAB_PRE", "1") == "1"
# round 6: the border-line sums that ca_scale_pre needs come out of the first convolution's epilogue (desc.border_pieces) instead of a
# launch of their own: one small launch per RCAB on the dependent chain instead of two.  EAVSR_RCAB_PRE_PIECES=0: A/B switch.
RCAB_PRE_PIECES = _os.environ.get("EAVSR_RCAB_PRE_PIECES", "1") == "1"


def set_rcab_pre(on: bool) -> None:
    global RCAB_PRE
    RCAB_PRE = bool(on)
# training: one autograd node per RCAB (autograd._RcabFn); EAVSR_RCAB_ONE_NODE=0: the per-op nodes of rounds 1-4
RCAB_ONE_NODE = _os.environ.get("EAVSR_RCAB_ONE_NODE", "1") != "0"
FUSE_CA_INTO_CONV = _os.environ.get("EAVSR_FUSE_CA", "0") == "1"
# One kernel per pyramid level of the residual-flow refinement (eavsr_flow_level_f32: front end + 64 -> 6 heads + affine +
# 18 -> 2 conv, only the two inputs and the 2-channel flow touch HBM) instead of four launches.  Correct (goldens G2 / G5,
# tests/test_hip_ops.py) but OFF by default: measured 28.5 ms per 2-clip forward against 13.0 ms for the four launches --
# a tile's 64 channel steps are serial inside one 4-wave workgroup (4 barriers each) and the 240 tiles of a 2 x 180 x 320
# launch leave no second workgroup per CU to hide them, while the un-fused kernels run 64x more workgroups.  EAVSR_FUSE_LEVEL=1
# / set_fuse_flow_level(True) turns it on (DESIGN.md has the analysis and what a channel-parallel version would need).
FUSE_FLOW_LEVEL = _os.environ.get("EAVSR_FUSE_LEVEL", "0") == "1"


def set_fuse_flow_level(on: bool) -> None:
    global FUSE_FLOW_LEVEL
    if on:
        ops.require_lab("the one-kernel-per-pyramid-level form (eavsr_flow_level_f32)")
    FUSE_FLOW_LEVEL = bool(on)


# In the 16-bit modes the predictor's 5x5 heads run on the 16-bit matrix pipe as well (csrc/conv5_h16.hip); EAVSR_HEADS_16BIT=0
# keeps them on the fp32 Winograd kernel.
HEADS_IN_16BIT = _os.environ.get("EAVSR_HEADS_16BIT", "1") == "1"
# Optional 16-bit residual backbone: None (exact fp32, the default and the BASELINE headline), "bf16" or "fp16"
# (set_backbone_dtype / EAVSR_BACKBONE_DTYPE).  Only the RCAGroup internals change precision.
BACKBONE_DTYPE = _os.environ.get("EAVSR_BACKBONE_DTYPE") or None
# conv -> ReLU -> conv of an RCAB as ONE launch in the 16-bit modes (eavsr_rcab_convs_h16, csrc/rcab_h16.hip: streamed weights, the
# intermediate in LDS; r bit-identical to the two launches).  OPT-IN (EAVSR_RCAB_H16_FUSED=1): back to back it is 49.7 us against
# 52.3 for the two launches at 4 x 64 x 256 x 256 (25.3 against 31.0 at 2 x 180 x 320, 94.1 against 81.7 at 1 x 540 x 960), but
# configs[2]'s two-stream step is 197.3 ms with it against 195.3 without (DESIGN.md 3.6 has the per-phase stamps).
RCAB_H16_FUSED = _os.environ.get("EAVSR_RCAB_H16_FUSED", "0") == "1"


def set_rcab_h16_fused(on: bool) -> None:
    global RCAB_H16_FUSED
    if on:
        ops.require_lab("the one-launch 16-bit RCAB (eavsr_rcab_convs_h16)")
    RCAB_H16_FUSED = bool(on)


# The RCAB's attention computed BEFORE its second convolution and the tail `res * y + x` folded into that convolution's epilogue
# (16-bit modes; csrc/ca.hip eavsr_ca_scale_pre_h16 + eavsr_conv3x3_c64_h16_res): no scale_residual_h16 launch -- three 128-byte-
# per-pixel streams per RCAB.  EAVSR_RCAB_H16_PRE=0 keeps conv, conv, ca_scale, scale_residual (A/B switch).
RCAB_H16_PRE = _os.environ.get("EAVSR_RCAB_H16_PRE", "1") == "1"


def set_rcab_h16_pre(on: bool) -> None:
    global RCAB_H16_PRE
    RCAB_H16_PRE = bool(on)
if BACKBONE_DTYPE is not None:
    ops.set_conv3_h16(BACKBONE_DTYPE)


def set_backbone_dtype(dtype):
    """None -> fp32 everywhere; 'bf16' / 'fp16' -> 16-bit NHWC activations inside every RCAGroup."""
    global BACKBONE_DTYPE
    if dtype is not None:
        ops.h16_code(dtype)
    BACKBONE_DTYPE = dtype
    ops.set_conv3_h16(dtype)      # ... and the plain 3x3 convolutions outside them (first conv of a backbone, encoder): csrc/conv3_h16.hip


import contextlib as _contextlib


@_contextlib.contextmanager
def backbone_dtype(dtype):
    """`with networks.backbone_dtype("bf16"): y = net(x)` -- the 16-bit modes for the body only; the previous setting is
    restored on exit."""
    prev = BACKBONE_DTYPE
    set_backbone_dtype(dtype)
    try:
        yield
    finally:
        set_backbone_dtype(prev)


# ---- the range census of the 16-bit modes (addendum) ----------------------------------------------------------------
# None (the default: every launch and byte is what it was), "report", "raise" or "bf16": set_backbone_check / backbone_check /
# EAVSR_BACKBONE_CHECK / opt.backbone_check.  While one is set, every launch of a 16-bit op counts what it rounds (ops._launch,
# ops.RangeCensus) and EAVSRP.forward / forward_long read the counts as `BackboneWindow` orders it.
BACKBONE_CHECKS = ("report", "raise", "bf16")


def check_backbone_check(mode, dtype="unknown", who: str = "backbone_check"):
    """`mode` beside the backbone dtype it would run with (left out: the spelling alone): None | "report" (count, read when the call
    ends) | "raise" (read before anything leaves, refuse a window that holds inf / NaN or overflowed) | "bf16" (likewise, and run such
    a window of an fp16 backbone again in bf16).  Refused: anything else, a check without a 16-bit backbone, "bf16" where the
    backbone is not fp16, any check with the one-launch RCAB of the lab build (its intermediate never leaves LDS)."""
    if mode is None:
        return None
    if not isinstance(mode, str) or mode not in BACKBONE_CHECKS:
        raise ValueError(f"{who} {mode!r}: None, 'report', 'raise' or 'bf16'")
    if dtype == "unknown":
        return mode
    if dtype is None:
        raise ValueError(f"{who} {mode!r} without a 16-bit backbone (set_backbone_dtype('fp16' / 'bf16')): the census is taken where "
                         "activations are rounded to 16 bits")
    if mode == "bf16" and ops.h16_code(dtype) != ops.h16_code("fp16"):
        raise ValueError(f"{who} 'bf16' with the {dtype!r} backbone: the fallback is from an fp16 backbone")
    if RCAB_H16_FUSED:
        raise ValueError(f"{who} {mode!r} with RCAB_H16_FUSED: the one-launch RCAB keeps its intermediate in LDS, where nothing can "
                         "count it (set_rcab_h16_fused(False))")
    return mode


BACKBONE_CHECK = check_backbone_check(_os.environ.get("EAVSR_BACKBONE_CHECK") or None, who="EAVSR_BACKBONE_CHECK")
# where the mode came from: "env" (read above: an environment set for inference runs does not stop training -- a call under autograd
# ignores it) or "call" (set_backbone_check / backbone_check: such a call under autograd is refused)
_BACKBONE_CHECK_FROM = "env"


def set_backbone_check(mode) -> None:
    """None | "report" | "raise" | "bf16": the range census of the 16-bit backbone (`check_backbone_check`), for every EAVSRP.forward /
    forward_long call from here on.  Checked against the backbone dtype of the moment here, and again at every call."""
    global BACKBONE_CHECK, _BACKBONE_CHECK_FROM
    BACKBONE_CHECK = check_backbone_check(mode, BACKBONE_DTYPE, "set_backbone_check")
    _BACKBONE_CHECK_FROM = "call"


@_contextlib.contextmanager
def backbone_check(mode):
    """`with networks.backbone_check("report"): sr = net(x)` -- the check for the body only; the previous setting is restored on exit,
    also when the body raises."""
    global BACKBONE_CHECK, _BACKBONE_CHECK_FROM
    prev = BACKBONE_CHECK, _BACKBONE_CHECK_FROM
    set_backbone_check(mode)
    try:
        yield
    finally:
        BACKBONE_CHECK, _BACKBONE_CHECK_FROM = prev


def _short_dtype(dtype) -> str:
    return "fp16" if ops.h16_code(dtype) == 1 else "bf16"


def active_backbone_check():
    """(mode, backbone dtype as "fp16" / "bf16") of a call that starts now, or None without a check (or with one that only the
    environment set, under autograd: training reads neither the option nor the environment) -- the refusals of
    `check_backbone_check`, and of a check under gradients or, where it synchronises, under stream capture"""
    if BACKBONE_CHECK is None or (_BACKBONE_CHECK_FROM == "env" and torch.is_grad_enabled()):
        return None
    mode = check_backbone_check(BACKBONE_CHECK, BACKBONE_DTYPE)
    if torch.is_grad_enabled():
        raise ValueError(f"backbone_check {mode!r} under autograd: the census belongs to the 16-bit inference modes (torch.no_grad())")
    if mode != "report" and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise ValueError(f"backbone_check {mode!r} under stream capture: it reads the census back, which synchronises ('report' does not)")
    return mode, _short_dtype(BACKBONE_DTYPE)


def tripped(sites) -> List[dict]:
    """the sites that hold a non-finite word or rounded a finite value to inf, in the order in which they first did ('tripped_at',
    the census's count of launches: time steps share rows, so a later step's input may trip a site that is earlier in call order)"""
    return sorted((s for s in sites if s["nonfinite"] > 0 or s["overflow"] > 0), key=lambda s: s.get("tripped_at", 0))


class BackboneRangeError(ValueError):
    """a window (or a chunk of its tail) whose activations do not fit the 16-bit backbone (`backbone_check("raise")`); `entry` is the
    call's census entry, `site` the site that tripped first IN TIME (`tripped`: the smallest 'tripped_at'; time steps share rows, so a
    later step's poisoned input trips sites that are earlier in call order than the one that left the range)"""

    def __init__(self, entry: dict, where: str):
        self.entry, self.site = entry, tripped(entry["sites"])[0]
        s = self.site
        super().__init__(f"{entry['asked']} backbone out of range in {where} of a window of {entry['frames']} frames of "
                         f"{entry['size'][0]} x {entry['size'][1]} -- first at {s['site']}: max |x| {s['max_abs']:.6g}, "
                         f"{s['nonfinite']} non-finite, {s['overflow']} overflowed of {s['elements']} "
                         f"({len(tripped(entry['sites']))} sites in all; nothing of it has reached the sink; "
                         "backbone_check('bf16') runs such a window in bf16)")


class BackboneWindow:
    """The order of one checked EAVSRP call -- pure host code over callables, as `framestore.checked_window`.  `stages(run)` runs
    stages 1-2 of `forward_long` (or the whole of `forward`), `tail(first_frame, run)` one chunk of stage 3, `close()` ends the call
    and appends its entry to `log`.  `open_census(dtype)` makes the object the launches count into (its `read()` returns the sites so
    far, cumulatively, and is the one synchronisation); `counting(census)` and `as_dtype(dtype)` are context managers: the
    launches of the body count into `census` / run under that backbone dtype.
    "report": one census for the whole call, read in `close`.  "raise" / "bf16": read behind `stages` and behind every `tail`, before
    its result is returned -- so before the sink sees it.  Where new counts of non-finite or overflowed elements have appeared:
    "raise" appends the entry and raises `BackboneRangeError`; "bf16" runs `run` again under `as_dtype("bf16")` (counted into a second,
    bf16 census: 'sites_used') -- behind `stages` the rest of the call stays in bf16 ('fallback'), behind a `tail` that chunk alone
    ('tail_fallback' gains its first frame).  Which site tripped first is the census's to say: every site's record carries
    'tripped_at', the count of counting launches at which its row first held inf / NaN or an overflow (`ops.RangeCensus`, the
    one-lane stamp launch behind every count); `tripped` orders by it."""

    def __init__(self, mode: str, dtype: str, about: dict, log: list, open_census=None, counting=None, as_dtype=None):
        self.mode, self.log = mode, log
        self.open_census = open_census or (lambda dt: ops.RangeCensus(dt, about.get("device", "cuda")))
        self.counting, self.as_dtype = counting or ops.range_census, as_dtype or backbone_dtype
        self.entry = dict(asked=dtype, used=dtype, fallback=False, tail_fallback=[],
                          **{k: v for k, v in about.items() if k != "device"}, sites=None)
        self.census, self.census_used, self._bad = self.open_census(dtype), None, 0

    def _new_trips(self) -> bool:
        self.entry["sites"] = self.census.read()
        bad = sum(s["nonfinite"] + s["overflow"] for s in self.entry["sites"])
        new, self._bad = bad > self._bad, bad
        return new

    def _in_bf16(self, run):
        if self.census_used is None:
            self.census_used = self.open_census("bf16")
        with self.as_dtype("bf16"), self.counting(self.census_used):
            return run()

    def _refuse(self, where: str):
        self.log.append(self.entry)
        raise BackboneRangeError(self.entry, where)

    def stages(self, run, rerun=None):
        """`rerun`: what runs in bf16 where `run` tripped (`forward_long`: the same stages on a fresh store); None: `run` again"""
        self.entry.update(used=self.entry["asked"], fallback=False)      # (a window that is filled twice starts again)
        with self.counting(self.census):
            out = run()
        if self.mode == "report" or not self._new_trips():
            return out
        if self.mode == "raise":
            self._refuse("stages 1-2")
        del out
        self.entry.update(used="bf16", fallback=True)
        return self._in_bf16(rerun or run)

    def tail(self, first_frame: int, run):
        if self.entry["fallback"]:
            return self._in_bf16(run)
        with self.counting(self.census):
            out = run()
        if self.mode == "report" or not self._new_trips():
            return out
        if self.mode == "raise":
            self._refuse(f"the tail of the chunk at frame {first_frame}")
        del out
        self.entry["tail_fallback"].append(int(first_frame))
        return self._in_bf16(run)

    def close(self):
        if self.mode == "report":
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                # a captured call launches nothing yet: the entry keeps the census, `entry['pending'].read()` after a replay
                self.entry["pending"] = self.census
            else:
                self.entry["sites"] = self.census.read()
        if self.census_used is not None:
            self.entry["sites_used"] = self.census_used.read()
        self.log.append(self.entry)
        return self.entry


def range_summary(log) -> dict:
    """one line over the entries of `EAVSRP.backbone_census`: the worst site (the smallest headroom; the first one that tripped
    where one did), its largest |x| and headroom, the totals of the counts, and the windows that fell back"""
    sites = [s for e in log for s in (e["sites"] or [])]
    # ('tripped_at' counts from 1 in every window's census: the first window that tripped, then the first site in it)
    bad = next((tripped(e["sites"]) for e in log if e["sites"] and tripped(e["sites"])), [])
    worst = bad[0] if bad else min(sites, key=lambda s: s["headroom"], default=None)
    out = {"windows": len(log), "worst_site": None if worst is None else worst["site"],
           "max_abs": 0.0 if worst is None else worst["max_abs"], "headroom": float("inf") if worst is None else worst["headroom"],
           "fallbacks": [i for i, e in enumerate(log) if e["fallback"]],
           "tail_fallbacks": [(i, f) for i, e in enumerate(log) for f in e["tail_fallback"]]}
    out.update({k: sum(s[k] for s in sites) for k in ("nonfinite", "overflow", "subnormal")})
    return out


TRAIN_PRECISIONS = ops.TRAIN_PRECISIONS


def set_train_precision(mode: str) -> None:
    """The opt-in bf16 TRAINING mode, in the spirit of torch.set_float32_matmul_precision("medium"): "fp32" (the default, from
    EAVSR_TRAIN_PRECISION: every convolution exact) or "bf16".  Anything else raises ValueError.

    Scope of "bf16": the 3x3 64 -> 64 convolutions that autograd RECORDS (autograd._ConvFn and _RcabFn: RCABlock's convolutions
    in training), their backward's input-gradient convolutions and their weight gradients -- wherever the crop-sized kernel takes
    the launch (ops.x6s_takes: at most ops.X6S_MAX_TILES 8 x 32-pixel tiles; the weight gradient also needs w % 4 == 0).  There every
    operand is rounded once to bf16 (nearest even) and each k-step is one bf16 product with fp32 accumulation; bias, activation
    and residual stay fp32.  Everything else is exactly as in "fp32": no-grad forwards (inference, evaluation in the middle of
    training through eavsr_amd.harness), the Winograd launches of large crops, 5x5 / 7x7, DCNv2 and the grouped convolutions.
    The mode is read at each recorded forward; a GraphedTrainStep recaptures when it changes.  (bench.py's result line keeps
    reporting `dtype: f32`: that field names the backbone activations, not this mode.)"""
    ops.TRAIN_PRECISION = ops.check_precision(mode)


def get_train_precision() -> str:
    return ops.TRAIN_PRECISION


@_contextlib.contextmanager
def train_precision(mode: str):
    """`with networks.train_precision("bf16"): model.optimize_parameters()` -- the previous mode is restored on exit, also when
    the body raises."""
    prev = ops.TRAIN_PRECISION
    set_train_precision(mode)
    try:
        yield
    finally:
        ops.TRAIN_PRECISION = prev


def set_deterministic(flag: bool) -> None:
    """The opt-in DETERMINISTIC training mode, in the spirit of torch.use_deterministic_algorithms(True): when on, a training step is a
    pure function of (parameters, optimizer state, inputs, modes, shapes) on one GPU with one build -- loss, gradients and updated
    parameters are bitwise identical from run to run, eager or graphed.  The backward of flow_warp, of resize_bilinear_ac and of
    DCNv2 then compute their input gradients without float atomics (csrc/det_scatter.hip; every other backward reduction is
    fixed-order in both modes), and autograd.grad_sink groups a weight's uses into weight-gradient launches without looking at
    earlier backwards.  A DCNv2 backward without an atomic-free form (not 64 -> 64 channels in 8 groups, or
    EAVSR_DCN_BWD=columns) raises RuntimeError.  Off by default (EAVSR_DETERMINISTIC=0|1); also on whenever torch.are_deterministic_algorithms_enabled().
    Composes with set_train_precision("bf16").  Read at each recorded forward; a GraphedTrainStep recaptures when it changes.
    flag must be a bool (ValueError otherwise)."""
    if not isinstance(flag, bool):
        raise ValueError(f"set_deterministic: expected True or False, got {flag!r}")
    ops.DETERMINISTIC = flag


def get_deterministic() -> bool:
    """whether training runs in the deterministic mode: set_deterministic(True) / EAVSR_DETERMINISTIC=1, or torch's own switch"""
    return ops.deterministic_active()


@_contextlib.contextmanager
def deterministic(flag: bool = True):
    """`with networks.deterministic(): model.optimize_parameters()` -- the previous setting is restored on exit, also when the body
    raises."""
    prev = ops.DETERMINISTIC
    set_deterministic(flag)
    try:
        yield
    finally:
        ops.DETERMINISTIC = prev


class RCAGroup(nn.Module):
    def __init__(self, in_channels=64, out_channels=64, kernel_size=3, stride=1, padding=1, bias=True,
                 mode="CRC", reduction=16, nb=12):
        super().__init__()
        assert in_channels == out_channels
        if mode[0] in "RL":
            mode = mode[0].lower() + mode[1:]
        RG = [RCABlock(in_channels, out_channels, kernel_size, stride, padding, bias, mode, reduction)
              for _ in range(nb)]
        RG.append(conv(out_channels, out_channels, mode="C"))
        self.rg = nn.Sequential(*RG)

    def _forward_h16(self, x, dtype):
        """16-bit backbone (BASELINE configs[2] / [4]): NHWC bf16 / fp16 activations through the whole group,
        fp32 accumulation and fp32 channel-attention statistics; fp32 NCHW at the group's boundary."""
        blocks, last = list(self.rg)[:-1], self.rg[-1]
        hw = x.shape[2] * x.shape[3]
        xs = ops.to_nhwc_h16(x, dtype)
        for blk in blocks:
            c1, c2 = blk.res[0], blk.res[2]
            if RCAB_H16_FUSED and ops.rcab_convs_h16_preferred(xs):      # conv -> ReLU -> conv as ONE launch (csrc/rcab_h16.hip)
                r, partial = ops.rcab_convs_h16(xs, c1.weight, c1.bias, c2.weight, c2.bias, chan_partial=True)
            elif RCAB_H16_PRE and int(blk.ca.conv_du[0].weight.shape[0]) <= 8:      # (the kernel's hidden-unit bound)
                # the attention BEFORE the second convolution (its output's channel means are linear in sums of its input), the
                # tail `res * y + x` as that convolution's epilogue: no scale_residual launch (csrc/ca.hip, ops.ca_scale_pre_h16)
                # (round 6: the border-line sums the attention needs come out of the first convolution's epilogue: one small launch
                # per block on the dependent chain instead of two; EAVSR_RCAB_PRE_PIECES=0 keeps the border-sum launch)
                t, tpart, pieces = ops.conv3x3_c64_h16(xs, c1.weight, c1.bias, relu=True, chan_partial=True, border=True) \
                    if RCAB_PRE_PIECES else (*ops.conv3x3_c64_h16(xs, c1.weight, c1.bias, relu=True, chan_partial=True), None)
                du_a, du_b = blk.ca.conv_du[0], blk.ca.conv_du[2]
                scale = ops.ca_scale_pre_h16(t, tpart, c2.weight, c2.bias, du_a.weight, du_a.bias, du_b.weight, du_b.bias, border=pieces)
                xs = ops.conv3x3_c64_h16_res(t, c2.weight, c2.bias, xs, scale)
                continue
            else:
                t = ops.conv3x3_c64_h16(xs, c1.weight, c1.bias, relu=True)
                r, partial = ops.conv3x3_c64_h16(t, c2.weight, c2.bias, chan_partial=True)
            xs = ops.scale_residual_h16(r, blk.ca.scale_from_partial(partial, hw), xs)
        y = ops.conv3x3_c64_h16(xs, last.weight, last.bias)
        return ops.from_nhwc_h16(y, residual=x)

    def forward(self, x):
        blocks, last = list(self.rg)[:-1], self.rg[-1]
        if BACKBONE_DTYPE is not None and not AG.needs_grad(x, list(self.parameters())) and x.shape[1] == 64 and \
                all(isinstance(b, RCABlock) and len(b.res) == 3 and isinstance(b.res[1], _Act) and b.res[1].kind == "relu"
                    and tuple(b.res[0].weight.shape) == (64, 64, 3, 3) for b in blocks) and \
                tuple(last.weight.shape) == (64, 64, 3, 3):
            return self._forward_h16(x, BACKBONE_DTYPE)
        fuse = FUSE_CA_INTO_CONV and not AG.needs_grad(x, list(self.parameters())) and ops.ca_fusable(x, last.weight.shape[0]) and len(blocks) > 0 and all(
            isinstance(b, RCABlock) and len(b.res) == 3 and isinstance(b.res[1], _Act) and b.res[1].kind == "relu"
            for b in blocks)
        if not fuse:
            r = x
            for blk in blocks:
                r = blk(r)
            return last(r, residual=x)                              # conv, + x  (:480-482)
        # Fused chain: the tail `res * y + x` of block k (networks.py:463-464) is applied inside the first
        # conv of block k+1 (and inside the group's last conv), which also emits the new residual stream.
        hw = x.shape[2] * x.shape[3]
        xs, r, scale = x, None, None
        for blk in blocks:
            c1, c2 = blk.res[0], blk.res[2]
            if r is None:
                t = c1(xs, act="relu")
            else:
                t, xs = ops.conv2d(r, c1.weight, c1.bias, act="relu", ca=(scale, xs), ca_out=True)
            r, partial = c2(t, chan_partial=True)
            scale = blk.ca.scale_from_partial(partial, hw)
        return ops.conv2d(r, last.weight, last.bias, residual=x, ca=(scale, xs))


# --------------------------------------------------------------------------------------------
# encoder (networks.py:522-552) -- a caller of the path ("next" row f2), run on the same conv kernel
# --------------------------------------------------------------------------------------------
class ContrasExtractorLayer(nn.Module):
    """VGG16 conv1_1 .. conv3_1 without the two pools + tail conv.  The reference pulls
    torchvision's pretrained VGG16 at construction; torchvision is not part of this image, so the
    convs start from PyTorch's default init and real weights arrive through load_state_dict
    (same keys: encoder.model.conv{1_1,1_2,2_1,2_2,3_1}.*, encoder.tail.*)."""

    def __init__(self, n_feat=64):
        super().__init__()
        cfg = [("conv1_1", 3, 64), ("conv1_2", 64, 64), ("conv2_1", 64, 128), ("conv2_2", 128, 128),
               ("conv3_1", 128, 256)]
        od = OrderedDict()
        for i, (name, ci, co) in enumerate(cfg):
            od[name] = Conv2d(ci, co, 3, 1, 1)
            if i < len(cfg) - 1:
                od[name.replace("conv", "relu")] = _Act("relu")
        self.tail = Conv2d(256, n_feat, 3, 1, 1)
        self.model = nn.Sequential(od)
        self.register_buffer("mean", torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer("std", torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))

    def forward(self, batch):
        batch = (batch - self.mean) / self.std if batch.requires_grad else ops.normalize(batch, self.mean, self.std)
        return self.tail(_run_fused(self.model, batch))


def init_net(net, init_type="default", init_gain=0.02, gpu_ids=()):
    """networks.py:67-74 replacement: one process per GPU, so no DataParallel wrapper -- the module
    moves to gpu_ids[0] (or the current device) and is returned as is."""
    if init_type not in ("default", None):
        raise NotImplementedError("only init_type='default' (what the EAVSR scripts use) is supported")
    if len(gpu_ids) > 0:
        net.to(torch.device("cuda", gpu_ids[0]))
    return net
