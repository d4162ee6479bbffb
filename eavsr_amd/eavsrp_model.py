"""Drop-in counterparts of models/eavsrp_model.py (x4) and models/eavsrpx2_model.py (x2).

`EAVSRP(opt, spynet_pretrained=None).forward(lrs)` keeps the reference signature
((n,t,3,h,w) in [0,1] -> (n,t,3,s*h,s*w), eavsrp_model.py:202-240) and state_dict keys, and runs
the whole forward on libeavsr_hip.so kernels: the alignment / propagation hot path (MultiAdSTN,
DCNv2, flow_warp, fusion, 30-RCAB backbones) and, on the same conv kernel, the callers either
side of it (SPyNet, encoder, upsampling tail).  torch is used for memory, views, and a few
elementwise / pooling glue ops outside the hot loop.

One process drives one GPU (no nn.DataParallel: networks.init_net here does not wrap).
"""
from __future__ import annotations

import os
import time
from typing import Dict, List

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import autograd as AG
from . import framestore as FS
from . import networks as N
from . import ops

# EAVSR_PREPACK=0: every weight's packed forms at their first use (the A/B switch of ops.prepack_conv3_x6)
PREPACK = os.environ.get("EAVSR_PREPACK", "1") != "0"

# In the 16-bit modes the upsampling tail (conv + PixelShuffle stages, conv_hr, conv_last) runs on the 16-bit kernels as well;
# EAVSR_TAIL_16BIT=0 keeps it on the fp32 kernels (A/B switch).
TAIL_IN_16BIT = os.environ.get("EAVSR_TAIL_16BIT", "1") == "1"

# EAVSR_HOIST=0: the alignment predictors inside the recurrence, one time step at a time (the A/B switch of EAVSRP._predict_branch)
HOIST_PREDICTORS = os.environ.get("EAVSR_HOIST", "1") != "0"
# the predictor stack (front-end outputs + head channels of 2 t - 1 row blocks) above which a branch keeps the per-step form
HOIST_MAX_BYTES = int(os.environ.get("EAVSR_HOIST_MAX_BYTES", str(16 << 30)))

Tensor = torch.Tensor


# ---------------------------------------------------------------------------------------------
# flow_warp with the flow in NHWC (eavsrp_model.py:587-626)
# ---------------------------------------------------------------------------------------------
def flow_warp(x, flow, interpolation="bilinear", padding_mode="zeros", align_corners=True):
    """Warp `x` (n,c,h,w) by `flow` (n,h,w,2): [...,0] = x displacement, [...,1] = y, in pixels."""
    return AG.flow_warp(x, flow, padding_mode=padding_mode, flow_layout="nhwc", interpolation=interpolation,
                        align_corners=align_corners)


# ---------------------------------------------------------------------------------------------
# residual backbone (eavsrp_model.py:366-400)
class _FrameList(list):
    """a list of per-frame tensors (n, c, h, w) that may know the frame-major tensor (t*n, c, h, w) its items are views of"""

    def __init__(self, items, stacked=None):
        super().__init__(items)
        self.stacked = stacked


def _frame_major(frames) -> Tensor:
    st = getattr(frames, "stacked", None)
    return st if st is not None else torch.cat(list(frames), 0)


# ---------------------------------------------------------------------------------------------
def _clip_geometry(lrs, who: str):
    """(u8, hwc, n, t, h, w) of a clip handed to the inference path `who`: (n, t, 3, h, w), or 8-bit frames interleaved as
    (n, t, h, w, 3); anything else, and a call with gradients enabled, is refused under the caller's name"""
    if not isinstance(lrs, torch.Tensor) or lrs.dim() != 5:
        raise ValueError(f"{who}: lrs is an (n, t, 3, h, w) tensor (uint8: also (n, t, h, w, 3))")
    if torch.is_grad_enabled():
        raise RuntimeError(f"{who} is inference only: call it under torch.no_grad() (training runs `forward`)")
    u8 = lrs.dtype == torch.uint8
    hwc = u8 and lrs.shape[4] == 3 and lrs.shape[2] != 3
    h, w = (int(v) for v in (lrs.shape[2:4] if hwc else lrs.shape[3:]))
    return u8, hwc, int(lrs.shape[0]), int(lrs.shape[1]), h, w


class ResidualBlocksWithInputConv(nn.Module):
    """conv3x3(in -> out) + LeakyReLU(0.1) -> RCAGroup(nb=num_blocks).  `feat` may be a tensor or a
    list of tensors standing for their channel concatenation (the cat at eavsrp_model.py:322,353 is
    never materialised)."""

    def __init__(self, in_channels, out_channels=64, num_blocks=30):
        super().__init__()
        self.main = nn.Sequential(
            N.Conv2d(in_channels, out_channels, 3, 1, 1, bias=True),
            N._Act("lrelu", 0.1),
            N.RCAGroup(out_channels, out_channels, nb=num_blocks))

    def forward(self, feat):
        x = self.main[0](feat, act="lrelu", slope=0.1)
        return self.main[2](x)


# ---------------------------------------------------------------------------------------------
# SPyNet (eavsrp_model.py:402-585) -- caller of the path ("next" row f1); uses flow_warp(border)
# ---------------------------------------------------------------------------------------------
class ConvModule(nn.Module):
    """Key-compatible with mmcv.cnn.ConvModule(norm_cfg=None): .conv (+ fused ReLU)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, norm_cfg=None,
                 act_cfg=dict(type="ReLU")):
        super().__init__()
        assert norm_cfg is None and stride == 1 and padding == kernel_size // 2
        self.conv = N.Conv2d(in_channels, out_channels, kernel_size, stride, padding)
        self.with_activation = act_cfg is not None
        if self.with_activation:
            assert act_cfg["type"] == "ReLU"
            self.activate = N._Act("relu")

    def forward(self, x):
        return self.conv(x, act="relu" if self.with_activation else None)


class SPyNetBasicModule(nn.Module):
    def __init__(self):
        super().__init__()
        chans = [(8, 32), (32, 64), (64, 32), (32, 16), (16, 2)]
        self.basic_module = nn.Sequential(*[
            ConvModule(ci, co, 7, 1, 3, norm_cfg=None, act_cfg=dict(type="ReLU") if i < 4 else None)
            for i, (ci, co) in enumerate(chans)])

    def forward(self, tensor_input):
        return self.basic_module(tensor_input)


def load_checkpoint(module: nn.Module, path: str, strict: bool = True):
    """Reader for mmcv-style checkpoints ({'state_dict': ...} or a bare state dict), as
    mmcv.runner.load_checkpoint is used at eavsrp_model.py:421."""
    ck = torch.load(path, map_location="cpu")
    sd = ck.get("state_dict", ck) if isinstance(ck, dict) else ck
    sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
    module.load_state_dict(sd, strict=strict)
    return ck


class SPyNet(nn.Module):
    def __init__(self, pretrained):
        super().__init__()
        self.basic_module = nn.ModuleList([SPyNetBasicModule() for _ in range(6)])
        if isinstance(pretrained, str):
            load_checkpoint(self, pretrained, strict=True)
        elif pretrained is not None:
            raise TypeError(f"[pretrained] should be str or None, but got {type(pretrained)}.")
        self.register_buffer("mean", torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer("std", torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))

    def compute_flow(self, ref, supp):
        """eavsrp_model.py:433-488"""
        n, _, h, w = ref.size()
        ref = [ops.normalize(ref, self.mean, self.std)]
        supp = [ops.normalize(supp, self.mean, self.std)]
        for _ in range(5):
            ref.append(ops.avg_pool2(ref[-1]))
            supp.append(ops.avg_pool2(supp[-1]))
        ref, supp = ref[::-1], supp[::-1]
        flow = ref[0].new_zeros(n, 2, h // 32, w // 32)
        for level in range(len(ref)):
            if level == 0:
                flow_up = flow
            else:
                flow_up = ops.resize_bilinear_ac(flow, (flow.shape[2] * 2, flow.shape[3] * 2), 2.0)
            warped = ops.flow_warp(supp[level], flow_up, padding_mode="border")
            res = self.basic_module[level](ops.concat3(ref[level], warped, flow_up))
            flow = ops.add(flow_up, res)
        return flow

    def forward(self, ref, supp):
        """eavsrp_model.py:490-523"""
        h, w = ref.shape[2:4]
        w_up = w if (w % 32) == 0 else 32 * (w // 32 + 1)
        h_up = h if (h % 32) == 0 else 32 * (h // 32 + 1)
        # F.interpolate(.., size, 'bilinear', align_corners=False) both ways and the flow rescaling, as HIP kernels; a resize to
        # the same size is the identity (source coordinate = destination coordinate, weights 1 / 0) and is skipped
        if (h_up, w_up) != (h, w):
            ref = ops.resize_bilinear(ref, (h_up, w_up))
            supp = ops.resize_bilinear(supp, (h_up, w_up))
        flow = self.compute_flow(ref, supp)
        if (h_up, w_up) != (h, w):
            flow = ops.resize_bilinear(flow, (h, w), channel_mul=(float(w) / float(w_up), float(h) / float(h_up)))
        return flow


# ---------------------------------------------------------------------------------------------
# EAVSRP
# ---------------------------------------------------------------------------------------------
_PYR = ("spatial", "spatial_d2", "spatial_d4")


class EAVSRP(nn.Module):
    """eavsrp_model.py:121-364 (scale 4) / eavsrpx2_model.py:124-365 (scale 2, selected by
    opt.scale or the `scale` argument)."""

    def __init__(self, opt, spynet_pretrained=None, scale=None):
        super().__init__()
        self.opt = opt
        self.predict = getattr(opt, "predict", False)
        self.n_resblock = 30
        self.n_frame = getattr(opt, "n_frame", 7)
        self.n_feats = 64
        self.n_flow = getattr(opt, "n_flow", 5)
        self.scale = int(scale if scale is not None else getattr(opt, "scale", 4))
        if self.scale not in (2, 4):
            raise NotImplementedError("EAVSRP exists for x4 (eavsrp_model) and x2 (eavsrpx2_model)")
        # one entry per `forward_long` call that ran under a `cache_check` (addendum); the caller clears it
        self.cache_census = []
        # one entry per `forward` / `forward_long` call that ran under a `networks.backbone_check` (addendum); likewise
        self.backbone_census = []

        self.spynet = SPyNet(pretrained=spynet_pretrained)
        for p in self.spynet.parameters():
            p.requires_grad = False
        self.encoder = N.ContrasExtractorLayer(self.n_feats)

        self.deform_align = nn.ModuleDict()
        self.backbone = nn.ModuleDict()
        self.fusion = nn.ModuleDict()
        for i, module in enumerate(["backward_1", "forward_1", "backward_2", "forward_2"]):
            self.deform_align[module] = N.MultiAdSTN(opt, self.n_feats, self.n_feats, deformable_groups=8)
            self.backbone[module] = ResidualBlocksWithInputConv((2 + i) * self.n_feats, self.n_feats, self.n_resblock)
            self.fusion[module] = N.Conv2d(self.n_feats * 3, self.n_feats, 1, 1, 0, bias=True)

        self.reconstruction = ResidualBlocksWithInputConv(5 * self.n_feats, self.n_feats, 5)
        self.upsample1 = N.seq([N.conv(self.n_feats, self.n_feats * 4, mode="C"), nn.PixelShuffle(2)])
        if self.scale == 4:
            self.upsample2 = N.seq([N.conv(self.n_feats, self.n_feats * 4, mode="C"), nn.PixelShuffle(2)])
        self.conv_hr = N.Conv2d(64, 64, 3, 1, 1)
        self.conv_last = N.Conv2d(64, 3, 3, 1, 1)
        self.img_upsample = nn.Upsample(scale_factor=self.scale, mode="bilinear", align_corners=False)
        self.lrelu = N._Act("lrelu", 0.1)

    # -- flows -----------------------------------------------------------------------------
    def compute_flow(self, lrs, lr_tm=None):
        """eavsrp_model.py:179-200.  Both directions go through SPyNet as one batch."""
        n, t, c, h, w = lrs.shape
        # frame-major pairs (pair (frame i, clip b) -> row i n + b): the two frame runs are contiguous views of the frame-major
        # input, and a time step's flow `flows[:, i]` of the (n, t-1, 2, h, w) VIEWS returned here is contiguous, so that
        # `propagate` copies nothing (44 strided copies per forward in round 2)
        lr_tm = lrs.transpose(0, 1).reshape(t * n, c, h, w) if lr_tm is None else lr_tm
        m = n * (t - 1)
        lrs_1, lrs_2 = lr_tm[:m], lr_tm[n:]
        both = self.spynet(torch.cat([lrs_1, lrs_2], 0), torch.cat([lrs_2, lrs_1], 0))
        flows_backward = both[:m].view(t - 1, n, 2, h, w).transpose(0, 1)
        flows_forward = both[m:].view(t - 1, n, 2, h, w).transpose(0, 1)
        return flows_forward, flows_backward

    # -- forward ---------------------------------------------------------------------------
    def forward(self, lrs):
        chk = None if N.BACKBONE_CHECK is None else N.active_backbone_check()
        if chk is None:
            return self._forward(lrs)
        # under a `networks.backbone_check` (addendum): the same launches, each 16-bit one counted; the counts are read
        # before anything is returned ("raise" / "bf16") or once behind the last launch ("report")
        win = N.BackboneWindow(*chk, dict(frames=int(lrs.shape[1]), size=tuple(int(v) for v in lrs.shape[3:]), device=lrs.device),
                               self.__dict__.setdefault("backbone_census", []))
        out = win.stages(lambda: self._forward(lrs))
        win.close()
        return out

    def _forward(self, lrs):
        n, t, c, h, w = lrs.shape
        assert h >= 64 and w >= 64, (
            'The height and width of inputs should be at least 64, '
            f'but got {h} and {w}.')
        if not lrs.is_cuda:
            raise RuntimeError("eavsr_amd.EAVSRP runs on the GPU only (no CPU path); for a CPU reference use "
                               "the original repository with --gpu_ids -1")
        if torch.is_grad_enabled() and PREPACK and ops.x6s_takes(n, h, w):
            # training at a crop: the packed forms (forward + input-gradient) of every trainable 3x3 64 -> 64 weight in a handful of
            # launches here instead of one launch per weight and form at its first use (ops.prepack_conv3_x6)
            ops.prepack_conv3_x6([p_ for p_ in self.parameters() if p_.requires_grad and p_.dim() == 4 and tuple(p_.shape) == (64, 64, 3, 3)])
        # frame-major input so that every per-frame slice (of the input, the features, the flows) is contiguous
        lr_tm = lrs.transpose(0, 1).reshape(t * n, c, h, w)
        ops.range_mark("spynet")
        with torch.no_grad():
            flows_forward, flows_backward = self.compute_flow(lrs, lr_tm)

        ops.range_mark("encoder")
        f1 = self.encoder(lr_tm)                                   # :216
        f2, f4 = AG.pyramid(f1)                                    # :218-220
        feats: Dict[str, List[Tensor]] = {
            "spatial": _FrameList([f1[i * n:(i + 1) * n] for i in range(t)], f1),
            "spatial_d2": _FrameList([f2[i * n:(i + 1) * n] for i in range(t)], f2),
            "spatial_d4": _FrameList([f4[i * n:(i + 1) * n] for i in range(t)], f4),
        }
        for iter_ in (1, 2):
            for direction in ("backward", "forward"):
                module = f"{direction}_{iter_}"
                feats[module] = []
                flows = flows_backward if direction == "backward" else flows_forward
                feats = self.propagate(feats, flows, module)
        return self.upsample(lrs, feats, lr_tm)

    def _predict_branch(self, align, feats, flows, backward):
        """The alignment predictors of ALL time steps of one branch, ahead of its recurrence: in MultiAdSTN.forward
        (networks.py:597-631) everything in front of the warp of `feat_prop` reads the encoder pyramids, SPyNet's flows and the
        branch's weights only.  Returns (off1, heads1, off2, heads2) -- refined offsets (rows, 2, h, w) and head channels
        (rows, 15 D, h, w), frame-major; row block j of the first-order pair belongs to the time step whose flow is flows[:, j],
        row block j of the second-order pair to the step whose `flow_n1` is flows[:, j] (backward) / flows[:, j + 1] (forward) --
        or None where `propagate` keeps the per-step form: gradients, the 16-bit modes, the un-fused DCNv2 modes, pyramids that
        are not views of frame-major tensors, a stack beyond HOIST_MAX_BYTES.
        Every input is a contiguous run of rows of a frame-major tensor, so nothing is gathered; the refinement chains run once per
        order (t n and (t - 1) n images), their front ends write into ONE stack and the 5x5 heads are ONE launch over it."""
        n, t, _, h, w = flows.size()
        pyr = [getattr(feats[k], "stacked", None) for k in _PYR]
        if any(p_ is None for p_ in pyr) or len(feats["spatial"]) != t + 1:
            return None
        return self._predict_rows(align, pyr, flows.transpose(0, 1).reshape(t * n, 2, h, w), n, backward)      # (a view: compute_flow returns views of the frame-major flows)

    def _predict_rows(self, align, pyr, fl, n, backward):
        """`_predict_branch` on frame-major tensors: pyr = the three pyramid levels ((t + 1) n rows each), fl = the flows (t n rows)"""
        t, h, w = int(fl.shape[0]) // n, int(fl.shape[2]), int(fl.shape[3])
        if t < 1 or AG.needs_grad(fl, pyr, list(align.parameters())) or not align.can_split(pyr[0][:n], fl[:n]):
            return None
        rows1, rows2 = t * n, (t - 1) * n
        if (rows1 + rows2) * h * w * 4 * (self.n_feats + 15 * align.deform_groups) > HOIST_MAX_BYTES:
            return None
        lo = lambda rows: [p_[:rows] for p_ in pyr]             # frames 0 .. of every level
        hi = lambda rows: [p_[p_.shape[0] - rows:] for p_ in pyr]      # frames .. t
        stack = fl.new_empty(rows1 + rows2, self.n_feats, h, w)
        # first order: (cur = frame j, nbr = j + 1) backward, (cur = j + 1, nbr = j) forward, flow j
        cur, nbr = (lo(rows1), hi(rows1)) if backward else (hi(rows1), lo(rows1))
        off1, _ = align.predict_front(nbr, cur, fl, out=stack[:rows1])
        off2 = None
        if rows2:
            # second order: (cur = j, nbr = j + 2, flow_n1 = j, flow_n2 = j + 1) backward, (cur = j + 2, nbr = j, j + 1, j) forward
            cur, nbr = (lo(rows2), hi(rows2)) if backward else (hi(rows2), lo(rows2))
            f_n1, f_n2 = (fl[:rows2], fl[n:]) if backward else (fl[n:], fl[:rows2])
            flow_n2 = ops.add(f_n1, ops.flow_warp(f_n2, f_n1))                              # :309-310
            off2, _ = align.predict_front(nbr, cur, flow_n2, out=stack[rows1:])
        heads = align.heads_of(stack)
        return off1, heads[:rows1], off2, heads[rows1:]

    def propagate(self, feats, flows, module_name):
        """eavsrp_model.py:242-329."""
        n, t, _, h, w = flows.size()
        frame_idx = list(range(0, t + 1))
        flow_idx = list(range(-1, t))
        mapping_idx = list(range(0, len(feats["spatial"])))
        mapping_idx += mapping_idx[::-1]
        backward = "backward" in module_name
        if backward:
            frame_idx = frame_idx[::-1]
            flow_idx = frame_idx
        step = 1 if backward else -1
        align, fusion, backbone = self.deform_align[module_name], self.fusion[module_name], self.backbone[module_name]
        feat_prop = flows.new_zeros(n, self.n_feats, h, w)
        zeros = None
        # inference: the branch's features go straight into one frame-major buffer (frame idx -> rows idx*n ..), which is what the
        # tail consumes -- the list below holds views of it and `upsample` needs no torch.cat (5 x 0.4 GB per 2-clip forward)
        stacked = None
        if not AG.needs_grad(flows, feats["spatial"][0], list(backbone.parameters())):
            stacked = flows.new_empty(len(feats["spatial"]) * n, self.n_feats, h, w)
        # inference, fp32: the predictors of every time step first, in batched launches; the loop keeps warp + DCNv2 (`sample`)
        ops.range_mark(module_name + ".predict")      # (a census; the hoist applies to fp32 only today: nothing is counted under it)
        pred = self._predict_branch(align, feats, flows, backward) if (HOIST_PREDICTORS and t > 0) else None
        for i, idx in enumerate(frame_idx):
            ops.range_mark(module_name)      # (a census: every time step counts into the rows of the first)
            cur = [feats[k][mapping_idx[idx]] for k in _PYR]
            if i > 0 and pred is not None:
                off1, heads1, off2, heads2 = pred
                j = flow_idx[i]
                cond_n1 = align.sample(feat_prop, off1[j * n:(j + 1) * n], heads1[j * n:(j + 1) * n])
                if i > 1:
                    j = idx if backward else idx - 2
                    cond_n2 = align.sample(feats[module_name][-2], off2[j * n:(j + 1) * n], heads2[j * n:(j + 1) * n])
                else:
                    if zeros is None:
                        zeros = torch.zeros_like(cond_n1)
                    cond_n2 = zeros
                feat_prop = fusion([cond_n1, cur[0], cond_n2])                          # :313-314
            elif i > 0:
                nbr = [feats[k][mapping_idx[idx + step]] for k in _PYR]
                flow_n1 = flows[:, flow_idx[i]].contiguous()
                cond_n1 = align(nbr, cur, feat_prop, flow_n1)
                if i > 1:
                    feat_n2 = feats[module_name][-2]
                    nbr2 = [feats[k][mapping_idx[idx + 2 * step]] for k in _PYR]
                    flow_n2 = flows[:, flow_idx[i - 1]].contiguous()
                    flow_n2 = AG.add(flow_n1, AG.flow_warp(flow_n2, flow_n1))            # :309-310
                    cond_n2 = align(nbr2, cur, feat_n2, flow_n2)
                else:
                    if zeros is None:
                        zeros = torch.zeros_like(cond_n1)
                    cond_n2 = zeros
                feat_prop = fusion([cond_n1, cur[0], cond_n2])                          # :313-314
            others = [feats[k][idx] for k in feats if k not in _PYR and k != module_name]
            res = backbone([cur[0]] + others + [feat_prop])                             # :317-323
            # AG.add honours `out` only without autograd: as soon as one frame's sum carries a gradient (a frozen backbone
            # behind a trained alignment / fusion module, an earlier branch with gradients) the buffer is dropped for the whole
            # branch -- its rows would stay uninitialised and cut off from autograd -- and `upsample` concatenates the list
            if stacked is not None and AG.needs_grad(feat_prop, res):
                stacked = None
            feat_prop = AG.add(feat_prop, res, out=None if stacked is None else stacked[idx * n:(idx + 1) * n])
            feats[module_name].append(feat_prop)
        if backward:
            feats[module_name] = feats[module_name][::-1]
        feats[module_name] = _FrameList(feats[module_name], stacked)
        return feats

    def upsample(self, lqs, feats, lq_tm=None):
        """eavsrp_model.py:331-364, all t frames as one batch."""
        n, t = lqs.shape[:2]
        branches = [k for k in feats if k not in _PYR]
        srcs = [_frame_major(feats["spatial"])] + [_frame_major(feats[k]) for k in branches]
        if lq_tm is None:
            lq_tm = lqs.transpose(0, 1).reshape(t * n, *lqs.shape[2:])
        out = self._upsample_tm(srcs, lq_tm)
        return out.view(t, n, *out.shape[1:]).transpose(0, 1).contiguous()

    def _upsample_tm(self, srcs, lq_tm):
        """the tail on frame-major tensors: srcs = `spatial` and the four branches (rows, 64, h, w), lq_tm (rows, 3, h, w) ->
        (rows, 3, s h, s w).  `upsample` runs it on all t n rows, `forward_long` on a chunk of frames."""
        ops.range_mark("tail")
        hr = self.reconstruction(srcs)
        tail16 = (N.BACKBONE_DTYPE is not None and TAIL_IN_16BIT and self.n_feats == 64 and
                  not AG.needs_grad(hr, lq_tm, list(self.upsample1.parameters()) + list(self.conv_hr.parameters()) +
                                    list(self.conv_last.parameters()) + (list(self.upsample2.parameters()) if self.scale == 4 else [])))
        if tail16:
            # 16-bit modes (BASELINE configs[2] / [4]): the tail on the 16-bit backbone kernel -- every conv + PixelShuffle(2) stage as
            # four 64 -> 64 slices whose store pattern is the shuffle, conv_hr as it is, conv_last by packed dot products; the
            # activations between them 16-bit NHWC, the skip image and the result fp32
            hr = ops.to_nhwc_h16(hr, N.BACKBONE_DTYPE)
            u1 = self.upsample1[0]
            hr = ops.conv3x3_c64_h16_act(hr, u1.weight, u1.bias, act="lrelu", slope=0.1, pixel_shuffle2=True)
            if self.scale == 4:
                u2 = self.upsample2[0]
                hr = ops.conv3x3_c64_h16_act(hr, u2.weight, u2.bias, act="lrelu", slope=0.1, pixel_shuffle2=True)
            hr = ops.conv3x3_c64_h16_act(hr, self.conv_hr.weight, self.conv_hr.bias, act="lrelu", slope=0.1)
            skip = ops.resize_bilinear(lq_tm, (self.scale * lq_tm.shape[2], self.scale * lq_tm.shape[3]))
            return ops.conv3x3_c64to3_h16(hr, self.conv_last.weight, self.conv_last.bias, residual=skip)
        # conv -> PixelShuffle(2) -> LeakyReLU (:343-347): the activation commutes with the shuffle and the shuffle is the conv
        # kernel's own store pattern (the torch copy was 0.8 / 3.3 GB per 2-clip forward)
        hr = self.upsample1[0](hr, act="lrelu", slope=0.1, pixel_shuffle2=True)
        if self.scale == 4:
            hr = self.upsample2[0](hr, act="lrelu", slope=0.1, pixel_shuffle2=True)
        hr = self.conv_hr(hr, act="lrelu", slope=0.1)
        # nn.Upsample(scale_factor, 'bilinear', align_corners=False) (:158,359): source coordinate (dst + 0.5) / s - 0.5
        skip = (self.img_upsample(lq_tm) if lq_tm.requires_grad else
                ops.resize_bilinear(lq_tm, (self.scale * lq_tm.shape[2], self.scale * lq_tm.shape[3])))
        return self.conv_last(hr, residual=skip)                                     # :359-360

    # -- long clips ------------------------------------------------------------------------
    def forward_long(self, lrs, frame_chunk=None, cache="device", sink=None, emit=None, pad=None, window=None, transform=None,
                     cache_dtype=None, cache_check=None):
        """`forward` for a whole scene, inference only (call it under torch.no_grad(); it raises otherwise).

        The three stages that `forward` runs on all t n frames as one batch -- SPyNet on the frame pairs, the encoder with the
        pyramid, the reconstruction with the upsampling tail -- run over `frame_chunk` frames at a time (all n clips of those
        frames), so their activations no longer grow with t; `propagate` is a per-time-step recurrence already and keeps its
        arithmetic.  Each chunk is launched under `ops.route_batch(<the whole batch>)`: every convolution takes the kernel the
        whole batch would take, and the result is bit-identical to `forward(lrs)` (DESIGN 7b names the one route that is not
        pinned).  frame_chunk=None or >= t: one chunk, no pinning -- the launches of `forward`.

        cache="device": every per-frame tensor stays in device memory, as in `forward`.  cache="host": the `cpu_cache` of the
        BasicVSR family -- frames in pinned host memory, a device window of what the current and the next time step read, copies
        on one side stream (`framestore.HostStore`).  A copy changes no bits: both give the same result.

        lrs: (n, t, 3, h, w) fp32 in [0, 1] on the device, or uint8 -- (n, t, 3, h, w) or interleaved (n, t, h, w, 3), on the
        device or in (pinned) host memory -- converted chunk by chunk with `ops.u8_to_f32` (v / 255, the reference's
        `np.float32(img) / 255`), so that a host-resident scene crosses the link as bytes.

        sink: `sink(first_frame, sr_chunk)` is called once per finished chunk with sr_chunk (n, frames, 3, s h, s w); the SR clip is
        then never allocated as a whole and None is returned.  Without a sink: the (n, t, 3, s h, s w) tensor `forward` returns.

        emit=(a, b), 0 <= a < b <= t (`forward_segments`): stages 1 and 2 run on all t frames, stage 3 -- the
        reconstruction and the upsampling tail -- only on frames a .. b - 1.  The sink sees those frames alone, `first_frame` still
        counted from the start of `lrs`; without a sink the (n, b - a, 3, s h, s w) tensor is returned.  Stage 3 is then always
        launched under `ops.route_batch(t n)`, one chunk or not: b - a frames on their own could take another kernel than the t
        frames do, and the result is frames a .. b - 1 of the run without `emit`, bit for bit.  emit=None: today's path.

        pad="reflect" / "edge" (DESIGN 7i): frames of ANY size.  Where (H, W) = `segments.padded_size(h, w)` differs from (h, w) the
        ingest pads every frame at the bottom and right while it converts it (`ops.ingest_pad`, one launch per chunk, all three
        kinds of source; a host-resident uint8 clip still crosses the link as its unpadded bytes), everything downstream runs on
        H x W frames, and every SR chunk is cropped to (s h, s w) before the sink sees it or it is stored: the result is
        `forward_long(<the clip padded by hand>)[..., :s h, :s w]`, bit for bit.  Where the size needs no padding the launches are
        those of pad=None.  pad=None: today's path, the assert below and `ops.pyramid`'s ValueError for other sizes included.

        window=(y0, y1, x0, x1) (`forward_tiled`): the clip is the window [y0, y1) x [x0, x1) of `lrs`' frames -- h, w are
        the window's size from here on, and the ingest reads the window in place (`ops.ingest_window`, one launch per chunk, all three
        kinds of source, padding to `padded_size` with `pad` in the same launch where the window's size needs it).  Everything else,
        the crop included, is unchanged: the result is `forward_long(lrs[..., y0:y1, x0:x1].contiguous(), ...)`, bit for bit.
        window=None: today's launches.

        transform=k, 1 .. 7 (`forward_ensemble`): the network sees the clip under mode k of the eight flips / transposes
        (bit 0 hflip, bit 1 vflip, bit 2 transpose, in that order).  Every ingested chunk -- window and padding as above, in their one
        launch -- goes through `ops.dihedral(.., k)`, and at the tail the crop is `segments.valid_region`, where the transform has
        moved the frame's samples to (a view, taken whether or not the size needed padding).  The sink, or the result, holds the
        frames in the TRANSFORMED orientation: `forward_long(g_k(<the padded window>))[valid region]`, bit for bit.  transform=None
        or 0: today's launches and today's crop.

        cache_dtype="fp16" / "bf16" (or the torch dtypes): the store holds the pyramid levels and the branches' outputs in
        16 bits -- rounded to nearest even when they enter it (`ops.pack16`), widened when they leave it (`ops.unpack16`, everything a
        time step fetches in one launch; with cache="host" on the side stream, and half the bytes cross the link).  No compute kernel
        changes; what a step keeps in hand (the recurrence's state) is not rounded; flows and LR frames stay fp32.  The result is NOT
        bit-identical to `forward`: it is `forward_long` on a store that returns `x.to(dtype).to(torch.float32)`, bit for bit, and the
        same for both caches.  fp16 keeps 11 significant bits and overflows to inf above 65504; bf16 cannot overflow and keeps 8.
        cache_dtype=None: today's stores, launches and bytes.

        cache_check="report" / "raise" / "bf16" (addendum), with a `cache_dtype`: the packs of this call also count what the
        rounding did, per feature key (`ops.pack16_census`: the largest finite |x|, the non-finite inputs, the overflows to inf, the
        flushes to zero, the subnormal results), and the call appends one entry to `self.cache_census` -- a list the caller clears:
        {'asked', 'used', 'fallback', 'frames', 'size', 'keys': {key: `ops.census_record`}}.  Every pack of the call happens in stages
        1 and 2, before the first frame reaches the sink (`framestore.checked_window` is the order).  "report": the census is read
        back once, after stage 3; no synchronisation inside the call, and the frames are those of cache_check=None, bit for bit.
        "raise": it is read between stages 2 and 3, and a key that overflowed or held inf / NaN raises `framestore.CacheRangeError`
        (a ValueError) before the sink has seen anything of this call.  "bf16" (cache_dtype="fp16" only): read at the same point; where
        a key overflowed, the store is dropped and stages 1 and 2 run again on a bf16 store -- the result is then
        `forward_long(cache_dtype="bf16")`'s, bit for bit, the entry says 'fallback': True, 'used': "bf16", keeps the fp16 attempt's
        census under 'keys' and gains the bf16 run's under 'keys_used'; a call without overflow is cache_dtype="fp16"'s, bit for
        bit.  Non-finite inputs are reported but trigger no fallback: bf16 cannot cure them.  Per call, not sticky.
        cache_check=None: every launch and byte is what it was."""
        from .segments import check_pad, padded_size, valid_region
        if transform is not None and (isinstance(transform, bool) or not isinstance(transform, int) or not 0 <= transform <= 7):
            raise ValueError(f"forward_long: transform {transform!r}: a mode 0 .. 7, or None")
        transform = transform or None
        FS.check_cache(cache)
        cache_dtype = FS.check_cache_dtype(cache_dtype)
        cache_check = FS.check_cache_check(cache_check, cache_dtype)
        check_pad(pad, "forward_long: pad")
        u8, hwc, n, t, h, w = _clip_geometry(lrs, "forward_long")
        if window is not None:
            if len(window) != 4 or any(isinstance(v, bool) or not isinstance(v, int) for v in window):
                raise ValueError(f"forward_long: window {window!r}: integers (y0, y1, x0, x1)")
            y0, y1, x0, x1 = window = tuple(window)
            if not (0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w):
                raise ValueError(f"forward_long: window {window!r} does not lie inside frames of {h} x {w}")
            h, w = y1 - y0, x1 - x0
        device = self._clip_device(lrs)
        size = None      # (H, W) of the padded frames, where `pad` is set and the size needs it
        if pad is not None and padded_size(h, w) != (h, w):
            size = padded_size(h, w)
        assert size is not None or (h >= 64 and w >= 64), (
            'The height and width of inputs should be at least 64, '
            f'but got {h} and {w}.')
        if frame_chunk is not None and int(frame_chunk) < 1:
            raise ValueError(f"frame_chunk {frame_chunk!r}: a positive number of frames, or None")
        fc = t if frame_chunk is None else min(int(frame_chunk), t)
        chunks = [(a, min(a + fc, t)) for a in range(0, t, fc)]
        single = len(chunks) == 1
        pin = (lambda rows: None) if single else (lambda rows: rows)      # one chunk IS the whole batch: nothing to pin
        if emit is not None:
            ea, eb = (int(v) for v in emit)
            if not 0 <= ea < eb <= t:
                raise ValueError(f"forward_long: emit {emit!r}: frames (a, b) with 0 <= a < b <= {t}")
        def make(dtype, census):      # (the calls without a census are the ones they were)
            if census:
                return FS.make_store(cache, n, t, device, dtype=dtype, census=True)
            return FS.make_store(cache, n, t, device) if dtype is None else FS.make_store(cache, n, t, device, dtype=dtype)

        def fill(store):
            # -- stage 1, per chunk: ingest, the flows of the chunk's frame pairs, encoder + pyramid
            last = None      # the previous chunk's last frame (first frame of this chunk's first pair)
            for a, b in chunks:
                lr_c = self._ingest(lrs, a, b, device, hwc, pad, size, window)
                if transform is not None:
                    lr_c = ops.dihedral(lr_c, transform)
                store.put_range("lr", a, lr_c)
                seq = lr_c if last is None else torch.cat([last, lr_c], 0)
                m = int(seq.shape[0]) - n      # rows of this chunk's pairs: (frame j, frame j + 1), j = first .. first + m / n - 1
                if m > 0:
                    lrs_1, lrs_2 = seq[:m], seq[n:]
                    ops.range_mark("spynet")
                    with ops.route_batch(pin(2 * n * (t - 1))):
                        both = self.spynet(torch.cat([lrs_1, lrs_2], 0), torch.cat([lrs_2, lrs_1], 0))
                    first = a if last is None else a - 1
                    store.put_range("flow_backward", first, both[:m])
                    store.put_range("flow_forward", first, both[m:])
                ops.range_mark("encoder")
                with ops.route_batch(pin(t * n)):
                    f1 = self.encoder(lr_c)
                    f2, f4 = AG.pyramid(f1)
                for key, val in zip(_PYR, (f1, f2, f4)):
                    store.put_range(key, a, val)
                last = lr_c[-n:]
                del lr_c, seq, f1, f2, f4

            # -- stage 2: the four branches, one time step at a time
            branches = []
            for iter_ in (1, 2):
                for direction in ("backward", "forward"):
                    module = f"{direction}_{iter_}"
                    self._propagate_long(store, module, list(branches), n, t, hoist=single)
                    branches.append(module)
            return branches

        def drain(store, branches):
            # -- stage 3, per chunk: reconstruction + upsampling tail
            keys = ["spatial"] + branches + ["lr"]
            out = None
            if emit is None:
                tail, pin_tail, base, single_tail = chunks, pin, 0, single
            else:      # the chunks' parts inside [ea, eb); always pinned: fewer rows than t n must not choose another kernel
                tail = [(max(a, ea), min(b, eb)) for a, b in chunks if max(a, ea) < min(b, eb)]
                pin_tail, base, single_tail = (lambda rows: rows), ea, len(tail) == 1
            for key in keys:
                store.prefetch_range(key, *tail[0])
            for ci, (a, b) in enumerate(tail):
                tensors = [store.get_range(key, a, b) for key in keys]
                if ci + 1 < len(tail):      # (host cache: the next chunk's copies overlap this chunk's kernels)
                    for key in keys:
                        store.prefetch_range(key, *tail[ci + 1])
                def run_tail(tensors=tensors):
                    with ops.route_batch(pin_tail(t * n)):
                        return self._upsample_tm(tensors[:-1], tensors[-1])
                sr = run_tail() if win is None else win.tail(a, run_tail)
                del tensors, run_tail
                sr = sr.view(b - a, n, *sr.shape[1:]).transpose(0, 1)
                if transform is not None:      # where mode k has moved the frame's samples to, inside its (transposed: s W x s H) SR frame
                    r0, r1, c0, c1 = valid_region(transform, h, w, *(size or (h, w)), self.scale)
                    sr = sr[..., r0:r1, c0:c1]
                elif size is not None:      # the crop: a view here, one copy of the chunk's output where it is made contiguous / stored below
                    sr = sr[..., :self.scale * h, :self.scale * w]
                if sink is not None:      # (`forward_tiled`'s own sink blends the view as it stands: `ops.tile_blend` reads strides)
                    sink(a, sr if getattr(sink, "takes_views", False) else sr.contiguous())
                elif single_tail:
                    out = sr.contiguous()
                else:
                    if out is None:
                        out = sr.new_empty((n, tail[-1][1] - base) + tuple(sr.shape[2:]))
                    out[:, a - base:b - base] = sr
                del sr
            return out

        win = None
        if N.BACKBONE_CHECK is not None and N.active_backbone_check() is not None:
            # under a `networks.backbone_check` (addendum): stages 1-2 and every chunk's tail run as `BackboneWindow`
            # orders them.  `checked_window` owns a `framestore.StoreBox`: a window that falls back drops the store of its fp16
            # attempt and fills a fresh one IN the box, so the cache census, `finish` and stage 3 all act on the store that was used
            win = N.BackboneWindow(*N.active_backbone_check(), dict(frames=t, size=(h, w), device=device),
                                   self.__dict__.setdefault("backbone_census", []))
            make0, fill0, drain0 = make, fill, drain

            def make(dtype, census):
                return FS.StoreBox(lambda: make0(dtype, census))

            def fill(box):
                def run():
                    return fill0(box.store)

                def again():
                    box.renew()      # (the fp16 attempt's store goes before the bf16 run's is taken)
                    return fill0(box.store)
                return win.stages(run, again)

            def drain(box, branches):
                return drain0(box.store, branches)

        def finish(out):
            if win is not None:
                win.close()
            return out
        if cache_check is None:      # make, fill, drain, finish
            return finish(FS.checked_window(make, fill, drain, cache_dtype, None, None, None))
        return finish(FS.checked_window(make, fill, drain, cache_dtype, cache_check, dict(frames=t, size=(h, w)),
                                        self.__dict__.setdefault("cache_census", [])))

    def forward_segments(self, lrs, segments, frame_chunk=None, cache="device", sink=None):
        """A clip of any length as a sequence of `forward_long` calls: for every (start, stop, emit_start, emit_stop) of
        `segments` (`segments.plan_segments`) `forward_long(lrs[:, start:stop], emit=...)` runs and frames emit_start .. emit_stop - 1
        of the clip are taken from it -- each frame exactly what `forward_long` gives for it on its window, each emitted once, in
        increasing order.  What is resident follows the longest window, not t.  `frame_chunk` / `cache` are `forward_long`'s;
        `sink(first_frame, sr_chunk)` sees frame numbers of `lrs`.  Without a sink: the assembled (n, t, 3, s h, s w) tensor.
        Frames of any size: `forward_segments_padded`."""
        return self.forward_segments_padded(lrs, segments, None, frame_chunk=frame_chunk, cache=cache, sink=sink)

    def forward_segments_padded(self, lrs, segments, pad, frame_chunk=None, cache="device", sink=None, cache_dtype=None, cache_check=None):
        """`forward_segments` for frames of any size: `pad` is `forward_long`'s -- "reflect" / "edge": every window is
        padded on the device while it is converted and its SR frames are cropped; None: `forward_segments` itself.  A method of its
        own: `forward_segments` keeps the parameter list it was published with.  `cache_dtype` is `forward_long`'s, for
        every window; it is also how `forward_segments` is called with a 16-bit cache (pad=None).  `cache_check` is `forward_long`'s
        too: one entry of `self.cache_census` per window, and with "bf16" each window falls back on its own."""
        from .segments import check_pad, check_plan
        check_pad(pad, "forward_segments_padded: pad")
        cache_dtype = FS.check_cache_dtype(cache_dtype)
        cache_check = FS.check_cache_check(cache_check, cache_dtype)
        _, _, _, t, _, _ = _clip_geometry(lrs, "forward_segments")

        def segment(part, emit, part_sink, last):
            return self.forward_long(part, frame_chunk=frame_chunk, cache=cache, sink=part_sink, emit=emit, pad=pad,
                                     cache_dtype=cache_dtype, **_checked(cache_check))
        return self._over_plan(lrs, check_plan(t, segments), sink, segment)

    def _over_plan(self, lrs, plan, sink, segment):
        """The loop of `forward_segments_padded` and `forward_tiled` over a checked segment plan: for every (start, stop, ea, eb)
        `segment(lrs[:, start:stop], emit, part_sink, last)` produces frames ea .. eb - 1 of the clip, emit = (ea - start, eb - start)
        counted inside the window as `forward_long` counts them.  With a sink, `part_sink` is the sink with its frame number moved
        from the window's to the clip's, the segment feeds it and nothing is returned; without one the segment returns its
        (n, eb - ea, ...) frames, which are the result where the plan is one segment and are assembled into (n, t, ...) otherwise.
        `last`: no segment follows (what a segment hands a sink may then be a view of storage it would reuse)."""
        n, t = int(lrs.shape[0]), int(lrs.shape[1])
        out = None
        for si, (start, stop, ea, eb) in enumerate(plan):
            part_sink = None if sink is None else (lambda first, sr, start=start: sink(start + first, sr))
            sr = segment(lrs[:, start:stop], (ea - start, eb - start), part_sink, si + 1 == len(plan))
            if sink is None:
                if len(plan) == 1:
                    return sr
                if out is None:
                    out = sr.new_empty((n, t) + tuple(sr.shape[2:]))
                out[:, ea:eb] = sr
            del sr
        return out

    def forward_tiled(self, lrs, tile, overlap=32, segments=None, pad=None, frame_chunk=None, cache="device", sink=None, cache_dtype=None,
                      cache_check=None):
        """Frames of any resolution, inference only: the network runs on overlapped spatial tiles and the SR tiles are
        blended into the frame with a feathered partition of unity, so what is resident follows the tile's area, not the frame's.

        `tile` (an int or (rows, columns), LR pixels) and `overlap` give the plan (`segments.plan_tiles`: windows of one size in
        row-major order); `lrs`, `frame_chunk`, `cache`, `pad` and `sink` are `forward_long`'s, `segments` is `forward_segments`'
        plan (None: the whole clip as one window of frames).  Per segment a host-resident 8-bit window of frames is uploaded once,
        as bytes, and every tile reads it there; an fp32 accumulator (n, emitted frames, 3, s h, s w) is zeroed; for every tile in
        plan order `forward_long(window=..., emit=..., pad=pad)` runs with a sink that adds each SR chunk, as the view it is, to the
        accumulator (`ops.tile_blend` with the rows of `segments.tile_weights`); the accumulator is then handed to
        `sink(first_frame, chunk)` in `frame_chunk` pieces, or assembled and returned where there is no sink.  One accumulator
        serves all segments (a sink that keeps its chunks gets copies while another segment is still to come).

        Contract: the result is that blend -- tile order, weights, (wy wx) sr then the sum, each rounded to fp32 -- of `forward_long`
        on each hand-cropped window, bit for bit.  It is NOT the whole-frame result: flow, DCN offsets and the 120 residual blocks
        of a tile see the tile alone, and near a seam two such views are averaged.

        Where one tile covers the frame the call IS `forward_long` / `forward_segments_padded`: no accumulator, no blend.
        `cache_dtype` is `forward_long`'s, for every tile, and so is `cache_check`: one entry of `self.cache_census` per
        tile and segment; with "bf16" a tile that overflowed is blended from its bf16 run beside fp16 neighbours."""
        from .segments import check_pad, check_plan, check_tile, plan_tiles, tile_axis
        FS.check_cache(cache)
        cache_dtype = FS.check_cache_dtype(cache_dtype)
        cache_check = FS.check_cache_check(cache_check, cache_dtype)
        check_pad(pad, "forward_tiled: pad")
        u8, hwc, n, t, h, w = _clip_geometry(lrs, "forward_tiled")
        sides = check_tile(tile, "forward_tiled: tile")
        if sides is None:
            raise ValueError("forward_tiled: tile=None (the untiled call is `forward_long`)")
        tiles = plan_tiles(h, w, sides, overlap)      # refuses a bad tile / overlap before anything runs
        if frame_chunk is not None and int(frame_chunk) < 1:
            raise ValueError(f"frame_chunk {frame_chunk!r}: a positive number of frames, or None")
        plan = [(0, t, 0, t)] if segments is None else check_plan(t, segments)
        if len(tiles) == 1:      # the untiled call: `_video` decides between `forward_long` and the segment plan
            return self._video(lrs, segments, None, 32, pad, frame_chunk, cache, sink, cache_dtype, cache_check)
        rows, cols = tile_axis(h, sides[0], overlap), tile_axis(w, sides[1], overlap)
        return self._blended("forward_tiled", lrs, (0,), tiles, rows, cols, plan, pad, frame_chunk, cache, sink, cache_dtype, cache_check)

    def _blended(self, who, lrs, modes, tiles, rows, cols, plan, pad, frame_chunk, cache, sink, cache_dtype, cache_check=None):
        """The accumulator loop of `forward_tiled` (modes = (0,)) and `forward_ensemble`, which have checked every argument: `tiles` in
        `plan_tiles` order over the windows `rows` x `cols` of the two axes (one tile: the frame, read without a window; its
        weights are 1), `plan` a checked segment plan.  Per segment the window of frames is uploaded once, the accumulator view is
        zeroed, `forward_long` runs per tile and, inside a tile, per mode in increasing order with a `_Blend` sink, and the
        accumulator is drained to `sink` in `frame_chunk` pieces."""
        from .segments import ensemble_weight, tile_weights
        _, _, n, _, h, w = _clip_geometry(lrs, who)
        device = self._clip_device(lrs)
        s = self.scale
        # (rows of tiles, s th): row i serves every tile of row i.  wy' = fp32(wy * weight), rounded once, on the host; one mode: x 1
        wy = torch.from_numpy(tile_weights(h, rows, s) * ensemble_weight(modes)).to(device)
        wx = torch.from_numpy(tile_weights(w, cols, s)).to(device)
        per_frame = 3 * s * h * s * w
        store = torch.empty(n * max(eb - ea for _, _, ea, eb in plan) * per_frame, device=device, dtype=torch.float32)

        def segment(part, emit, part_sink, last):
            if not part.is_cuda:
                part = part.to(device, non_blocking=True)      # once per segment, as bytes: every tile and mode reads it on the device
            k = emit[1] - emit[0]
            acc = store[:n * k * per_frame].view(n, k, 3, s * h, s * w)
            acc.zero_()
            for ti, window in enumerate(tiles):
                for mode in modes:
                    blend = _Blend(acc, emit[0], mode, s * window[0], s * window[2], wy[ti // len(cols)], wx[ti % len(cols)])
                    self.forward_long(part, frame_chunk=frame_chunk, cache=cache, sink=blend, emit=emit, pad=pad,
                                      window=window if len(tiles) > 1 else None, transform=mode, cache_dtype=cache_dtype,
                                      **_checked(cache_check))
            if part_sink is not None:
                fc = k if frame_chunk is None else min(int(frame_chunk), k)
                for a in range(0, k, fc):
                    chunk = acc[:, a:a + fc]
                    part_sink(emit[0] + a, chunk.contiguous() if last else chunk.clone())
            return acc
        return self._over_plan(lrs, plan, sink, segment)

    def forward_video(self, lrs, segments=None, tile=None, tile_overlap=32, pad=None, frame_chunk=None, cache="device", sink=None):
        """The one dispatch between the inference paths (`harness.super_resolve`, `EAVSRPModel.forward`): `forward_tiled` where
        `tile` (None: untiled) cuts the frames into more than one tile, else `forward_segments_padded` where there is a segment
        plan (`segments`, as `forward_segments` takes it), else `forward_long`.  `pad`, `frame_chunk`, `cache` and `sink` are
        handed on; so is the result.  (With a 16-bit feature cache: `forward_cached`.)"""
        return self._video(lrs, segments, tile, tile_overlap, pad, frame_chunk, cache, sink, None)

    def _video(self, lrs, segments, tile, tile_overlap, pad, frame_chunk, cache, sink, cache_dtype, cache_check=None):
        """`forward_video`'s dispatch, with `forward_long`'s `cache_dtype` -- and `cache_check`, handed on only where one is set -- for
        whichever path is taken"""
        from .segments import check_tile, plan_tiles
        sides = check_tile(tile, "forward_video: tile")
        if sides is not None:
            h, w = _clip_geometry(lrs, "forward_video")[4:]
            if len(plan_tiles(h, w, sides, tile_overlap)) > 1:
                return self.forward_tiled(lrs, tile, overlap=tile_overlap, segments=segments, pad=pad, frame_chunk=frame_chunk,
                                          cache=cache, sink=sink, cache_dtype=cache_dtype, **_checked(cache_check))
        if segments is not None:
            return self.forward_segments_padded(lrs, segments, pad, frame_chunk=frame_chunk, cache=cache, sink=sink,
                                                cache_dtype=cache_dtype, **_checked(cache_check))
        return self.forward_long(lrs, frame_chunk=frame_chunk, cache=cache, sink=sink, pad=pad, cache_dtype=cache_dtype,
                                 **_checked(cache_check))

    def forward_cached(self, lrs, cache_dtype, ensemble=None, tile=None, overlap=32, segments=None, pad=None, frame_chunk=None,
                       cache="device", sink=None, cache_check=None):
        """`forward_ensemble` -- and through it `forward_video`, `forward_tiled`, `forward_segments_padded` and `forward_long` -- with
        the 16-bit feature cache of `forward_long(cache_dtype=...)` in every `forward_long` call it makes.  A method of
        its own: `forward_video`, `forward_ensemble` and `forward_segments` keep the parameter lists they were published with.
        ensemble=None: no ensemble.  cache_dtype=None IS `forward_ensemble` / `forward_video`.  Refused before anything runs: a
        `cache_dtype` that is not None, "fp16", "bf16" or one of the two torch dtypes.  `cache_check` is `forward_long`'s (DESIGN 7n,
        addendum), for every call made: each appends its own entry to `self.cache_census` and, with "bf16", falls back on its own --
        a tiled, segmented or ensembled run may mix fp16 and bf16 windows, and the entries say which.  Refused with the rest: an
        unknown value, a check without a `cache_dtype`, "bf16" beside a cache that is not fp16."""
        cache_dtype = FS.check_cache_dtype(cache_dtype)
        cache_check = FS.check_cache_check(cache_check, cache_dtype)
        if ensemble is None:
            return self._video(lrs, segments, tile, overlap, pad, frame_chunk, cache, sink, cache_dtype, cache_check)
        return self._ensemble(lrs, ensemble, tile, overlap, segments, pad, frame_chunk, cache, sink, cache_dtype, cache_check)

    def forward_ensemble(self, lrs, ensemble=8, tile=None, overlap=32, segments=None, pad=None, frame_chunk=None, cache="device",
                         sink=None):
        """Geometric self-ensemble, inference only: the clip runs under each mode of `ensemble` -- the flips and
        transposes of the frame, `segments.check_ensemble`: 2, 4 / "flips", 8 or an explicit sequence of modes -- and the results,
        each turned back, are averaged.  A method of its own: `forward_video` keeps the parameter list it was published with;
        `harness.super_resolve` and the model wrapper call this one where an ensemble is set.

        `forward_tiled`'s loop with the mode loop inside the tile loop: per segment a host-resident 8-bit window of frames is
        uploaded once; the fp32 accumulator (n, emitted frames, 3, s h, s w) is zeroed; for every tile in `plan_tiles` order (untiled:
        the one window, the frame, with weights 1) and inside it for every mode k in increasing order,
        `forward_long(window=..., emit=..., pad=pad, transform=k)` runs with a sink that adds inv_k of every SR chunk, as the view it
        is, to the accumulator (`ops.blend_dihedral`): acc = acc + ((wy' wx) inv_k(sr)), three separately rounded fp32 operations,
        wy' = fp32(wy / len(modes)) computed once on the host.  The accumulator then goes to `sink(first_frame, chunk)` in
        `frame_chunk` pieces, or is returned assembled.  One accumulator serves all segments.

        Contract: the result is that numpy blend of `forward_long` on each hand-cropped, hand-padded, hand-transformed clip, bit for
        bit.  The network is NOT equivariant -- SPyNet, the DCN offsets and the residual blocks see the orientation -- so the modes
        differ and this is their mean, not an equivariant network.  Nothing is claimed about quality: no trained weights exist
        in this project, and the gain a published "+" row reports cannot be measured here.

        A spec that is off, or the one mode 0, IS `forward_video(...)`: no accumulator, no blend.  (With a 16-bit feature cache:
        `forward_cached`.)"""
        return self._ensemble(lrs, ensemble, tile, overlap, segments, pad, frame_chunk, cache, sink, None)

    def _ensemble(self, lrs, ensemble, tile, overlap, segments, pad, frame_chunk, cache, sink, cache_dtype, cache_check=None):
        """`forward_ensemble`'s body, with `forward_long`'s `cache_dtype` and `cache_check` (checked by the caller) for every call it makes"""
        from .segments import check_ensemble, check_pad, check_plan, check_tile, plan_tiles, tile_axis
        modes = check_ensemble(ensemble, "forward_ensemble: ensemble")      # refused before anything runs
        FS.check_cache(cache)
        check_pad(pad, "forward_ensemble: pad")
        u8, hwc, n, t, h, w = _clip_geometry(lrs, "forward_ensemble")
        sides = check_tile(tile, "forward_ensemble: tile")
        tiles = [(0, h, 0, w)] if sides is None else plan_tiles(h, w, sides, overlap)
        if frame_chunk is not None and int(frame_chunk) < 1:
            raise ValueError(f"frame_chunk {frame_chunk!r}: a positive number of frames, or None")
        plan = [(0, t, 0, t)] if segments is None else check_plan(t, segments)
        if modes is None or modes == (0,):      # off: no accumulator, no blend
            return self._video(lrs, segments, tile, overlap, pad, frame_chunk, cache, sink, cache_dtype, cache_check)
        if len(tiles) == 1:      # the whole frame (no tile, or one that covers it): one window per axis
            rows, cols = [(0, h)], [(0, w)]
        else:
            rows, cols = tile_axis(h, sides[0], overlap), tile_axis(w, sides[1], overlap)
        return self._blended("forward_ensemble", lrs, modes, tiles, rows, cols, plan, pad, frame_chunk, cache, sink, cache_dtype, cache_check)

    def _clip_device(self, lrs):
        """the device a clip runs on: its own, or the network's for 8-bit frames in host memory; anything but a GPU is refused"""
        if lrs.dtype != torch.uint8 and not lrs.is_cuda:
            raise RuntimeError("eavsr_amd.EAVSRP runs on the GPU only (no CPU path); for a CPU reference use "
                               "the original repository with --gpu_ids -1")
        device = lrs.device if lrs.is_cuda else next(self.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("eavsr_amd.EAVSRP runs on the GPU only (no CPU path): a uint8 clip in host memory needs the "
                               "network on the GPU")
        return device

    def _ingest(self, lrs, a, b, device, hwc, pad=None, size=None, window=None):
        """frames a .. b of the clip as frame-major fp32 ((b - a) n, 3, h, w) on the device; with `size` = (H, W): padded to it at
        the bottom and right (`ops.ingest_pad`, mode `pad`) in the launch that converts them; with `window` = (y0, y1, x0, x1): that
        window of them, read in place by the launch that converts (and pads) it (`ops.ingest_window`)"""
        part = lrs[:, a:b]
        u8 = part.dtype == torch.uint8
        if u8 and not part.is_cuda:
            part = part.to(device, non_blocking=True)      # bytes cross the link, whole and unpadded (`forward_tiled` uploads once instead)
        part = part.transpose(0, 1).reshape((b - a) * part.shape[0], *part.shape[2:])
        if window is not None:
            y0, y1, x0, x1 = window
            H, W = (y1 - y0, x1 - x0) if size is None else size
            return ops.ingest_window(part, y0, x0, y1 - y0, x1 - x0, H, W, mode=pad or "reflect", hwc=hwc)
        if size is not None:
            return ops.ingest_pad(part, size[0], size[1], mode=pad, hwc=hwc)
        return ops.u8_to_f32(part, hwc=hwc) if u8 else part

    def _propagate_long(self, store, module_name, others, n, t, hoist=False):
        """`propagate` (eavsrp_model.py:242-329) on a frame store, inference only: the same launches per time step; what a step
        reads comes from the store, whose schedule (`framestore.propagate_reads` / `prefetch_schedule`) has it on the device by
        then, and the step's result goes back to it."""
        backward = "backward" in module_name
        order = list(range(t))[::-1] if backward else list(range(t))
        step = 1 if backward else -1
        fkey = FS.FLOW_KEYS[0] if backward else FS.FLOW_KEYS[1]
        align, fusion, backbone = self.deform_align[module_name], self.fusion[module_name], self.backbone[module_name]
        store.begin(FS.prefetch_schedule(FS.propagate_reads(t, backward, others)))
        feat_prop, zeros, hist = None, None, []
        # hoist (one chunk = `forward`'s launches, frames resident on the device): the branch's predictors ahead of its time loop, as
        # `propagate`.  A chunked run asked for activations that do not grow with t and the host cache keeps a window of frames on
        # the device: both stay with the per-step form
        pred = None
        ops.range_mark(module_name + ".predict")
        if hoist and HOIST_PREDICTORS and getattr(store, "hoists", store.cache == "device") and t > 1:
            pred = self._predict_rows(align, [store.get_range(k, 0, t) for k in _PYR], store.get_range(fkey, 0, t - 1), n, backward)
        for i, idx in enumerate(order):
            store.step(i)
            ops.range_mark(module_name)
            cur = [store.get(k, idx) for k in _PYR]
            if i == 0:
                feat_prop = cur[0].new_zeros(cur[0].shape[0], self.n_feats, *cur[0].shape[2:])
                store.new_branch(module_name, feat_prop)
            elif pred is not None:
                off1, heads1, off2, heads2 = pred
                j = idx if backward else idx - 1
                cond_n1 = align.sample(feat_prop, off1[j * n:(j + 1) * n], heads1[j * n:(j + 1) * n])
                if i > 1:
                    j = idx if backward else idx - 2
                    cond_n2 = align.sample(hist[-2], off2[j * n:(j + 1) * n], heads2[j * n:(j + 1) * n])
                else:
                    if zeros is None:
                        zeros = torch.zeros_like(cond_n1)
                    cond_n2 = zeros
                feat_prop = fusion([cond_n1, cur[0], cond_n2])                          # :313-314
            else:
                nbr = [store.get(k, idx + step) for k in _PYR]
                flow_n1 = store.get(fkey, idx if backward else idx - 1)
                cond_n1 = align(nbr, cur, feat_prop, flow_n1)
                if i > 1:
                    feat_n2 = hist[-2]
                    nbr2 = [store.get(k, idx + 2 * step) for k in _PYR]
                    flow_n2 = store.get(fkey, idx + 1 if backward else idx - 2)
                    flow_n2 = AG.add(flow_n1, AG.flow_warp(flow_n2, flow_n1))            # :309-310
                    cond_n2 = align(nbr2, cur, feat_n2, flow_n2)
                else:
                    if zeros is None:
                        zeros = torch.zeros_like(cond_n1)
                    cond_n2 = zeros
                feat_prop = fusion([cond_n1, cur[0], cond_n2])                          # :313-314
            res = backbone([cur[0]] + [store.get(k, idx) for k in others] + [feat_prop])   # :317-323
            feat_prop = AG.add(feat_prop, res, out=store.out_slot(module_name, idx))
            store.put(module_name, idx, feat_prop)
            hist = (hist + [feat_prop])[-2:]
            store.done(i)


class _Blend:
    """`EAVSRP._blended`'s sink: adds every SR chunk of one tile, as the view `forward_long` holds and in the orientation of mode k, to
    the accumulator -- inv_k on the load (`ops.blend_dihedral`; k = 0 is `ops.tile_blend`'s launch)"""
    takes_views = True

    def __init__(self, acc, first, k, Y0, X0, wy, wx):
        self.acc, self.first, self.k, self.Y0, self.X0, self.wy, self.wx = acc, first, k, Y0, X0, wy, wx

    def __call__(self, first_frame, sr):
        a = first_frame - self.first      # the chunk's first frame among the emitted ones
        b = a + int(sr.shape[1])
        n = int(self.acc.shape[0])
        if n == 1 or (a == 0 and b == int(self.acc.shape[1])):
            ops.blend_dihedral(self.acc[:, a:b], sr, self.k, self.Y0, self.X0, self.wy, self.wx)
        else:      # frames a .. b of several clips are not one contiguous block: clip by clip
            for i in range(n):
                ops.blend_dihedral(self.acc[i:i + 1, a:b], sr[i:i + 1], self.k, self.Y0, self.X0, self.wy, self.wx)


class EAVSRPx2(EAVSRP):
    """eavsrpx2_model.py's network (class EAVSRP there): one pixel-shuffle stage, x2 bilinear skip."""

    def __init__(self, opt, spynet_pretrained=None):
        super().__init__(opt, spynet_pretrained, scale=2)


# ---------------------------------------------------------------------------------------------
# model wrapper (eavsrp_model.py:18-119), inference side
# ---------------------------------------------------------------------------------------------
def get_scheduler(optimizer, opt):
    """models/networks.py:16-37: the four learning-rate policies of the reference's options, same constants."""
    from torch.optim import lr_scheduler
    policy = getattr(opt, "lr_policy", "step")
    if policy == "linear":
        def lambda_rule(epoch):
            return 1 - max(0, epoch - opt.niter) / max(1, float(opt.niter_decay))
        return lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda_rule)
    if policy == "step":
        return lr_scheduler.StepLR(optimizer, step_size=opt.lr_decay_iters, gamma=0.5)
    if policy == "plateau":
        return lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=0.2, threshold=0.01, patience=5)
    if policy == "cosine":
        return lr_scheduler.CosineAnnealingLR(optimizer, T_max=opt.niter, eta_min=0)
    raise NotImplementedError("lr [%s] is not implemented" % policy)


def make_optimizer(net: "EAVSRP", opt) -> torch.optim.Adam:
    """Adam with the reference's two parameter groups (eavsrp_model.py:45-59): the alignment modules at lr 1e-5, the
    rest at opt.lr -- both built from ALL of `net.parameters()` in registration order exactly as the reference builds
    them, the 60 frozen SPyNet tensors included.  Those never receive a gradient, so Adam skips them, but they count in
    the state_dict's parameter indices: an `EAVSRP_optimizer_Adam.pth` written by either implementation resumes in the
    other (base_model.py:251-270)."""
    align_ids = {id(p) for p in net.deform_align.parameters()}
    every = list(net.parameters())
    basic = [p for p in every if id(p) not in align_ids]
    align = [p for p in every if id(p) in align_ids]
    return torch.optim.Adam([{"params": basic}, {"params": align, "lr": 1e-5}], lr=getattr(opt, "lr", 1e-4),
                            betas=(getattr(opt, "beta1", 0.9), getattr(opt, "beta2", 0.999)),
                            weight_decay=getattr(opt, "weight_decay", 0.0))


def long_clip_options(opt=None):
    """(frame_chunk, cpu_cache) of the opt-in long-clip path: `opt.frame_chunk` (frames per chunk of the batched stages; None / 0 =
    off) and `opt.cpu_cache` (per-frame tensors in pinned host memory), each falling back to the environment where the options do
    not carry it -- EAVSR_FRAME_CHUNK=<positive integer>, EAVSR_CPU_CACHE=0|1.  Neither is among the reference's options."""
    from .segments import digits, one_of, read_option, whole_number

    def flag(value, who):
        if not isinstance(value, bool):
            raise ValueError(f"{who}={value!r}: True or False")
        return value
    fc = read_option(opt, "frame_chunk", "EAVSR_FRAME_CHUNK", whole_number(0, "a positive number of frames, or None"),
                     digits(1, "a positive number of frames")) or None
    cc = read_option(opt, "cpu_cache", "EAVSR_CPU_CACHE", flag, lambda text, who: one_of(("0", "1"), "0 or 1")(text, who) == "1",
                     default=False, empty_is_unset=False)      # (the one variable that, set, may not be empty)
    png_encoder_option(opt)      # validated with the others; read where frames are written (harness.super_resolve)
    png_decoder_option(opt)      # likewise; read where frames are read (harness.super_resolve, at every call)
    from .segments import segment_options
    segment_options(opt)         # likewise: opt.max_frames / segment_overlap / scene_cuts, read by harness.super_resolve at every call
    from .segments import pad_option
    pad_option(opt)              # likewise: opt.pad_frames, read by EAVSRPModel.forward and harness.super_resolve
    from .segments import tile_options
    tile_options(opt)            # likewise: opt.tile / tile_overlap, read by EAVSRPModel.forward and harness.super_resolve
    from .segments import ensemble_options
    ensemble_options(opt)        # likewise: opt.ensemble, read by EAVSRPModel.forward and harness.super_resolve
    cache_dtype_option(opt)      # likewise: opt.cache_dtype, read by EAVSRPModel.forward and harness.super_resolve
    cache_check_option(opt)      # likewise: opt.cache_check, read beside it
    backbone_check_option(opt)   # likewise: opt.backbone_check, read by EAVSRPModel.forward and harness.super_resolve (addendum)
    from .resize import out_size_option
    out_size_option(opt)         # likewise: opt.out_size, read by EAVSRPModel.forward and harness.super_resolve
    return fc, cc


def _checked(cache_check):
    """the keyword a `forward_long` call (or one of the methods that lead to it) gains under a `cache_check`; none without one: the
    call is then the call it was"""
    return {} if cache_check is None else {"cache_check": cache_check}


def cache_check_option(opt=None):
    """None, "report", "raise" or "bf16": what is done about the range of the 16-bit feature cache (`EAVSRP.forward_long(cache_check=...)`,
    DESIGN 7n addendum) -- `opt.cache_check`, falling back to the environment where the options do not carry it
    (EAVSR_CACHE_CHECK=report|raise|bf16), None -- no census -- where neither does.  The spelling alone is checked here; that a
    check needs a `cache_dtype`, and "bf16" an fp16 one, is refused where both are known (`framestore.check_cache_check`).  Not among
    the reference's options."""
    from .segments import one_of, read_option
    choices = one_of(FS.CACHE_CHECKS, "report, raise or bf16")

    def from_opt(value, who):
        if not isinstance(value, str):
            raise ValueError(f"{who}={value!r}: 'report', 'raise', 'bf16' or None")
        return one_of(FS.CACHE_CHECKS, "'report', 'raise', 'bf16' or None")(value, who)
    return read_option(opt, "cache_check", "EAVSR_CACHE_CHECK", from_opt, choices)


def backbone_check_option(opt=None):
    """None, "report", "raise" or "bf16": the range census of the 16-bit backbone (`networks.set_backbone_check`, DESIGN 3.6 addendum)
    -- `opt.backbone_check`, falling back to the environment where the options do not carry it
    (EAVSR_BACKBONE_CHECK=report|raise|bf16), None -- no census -- where neither does.  The spelling alone is checked here; that a
    check needs a 16-bit backbone, and "bf16" an fp16 one, is refused where the call is made (`networks.check_backbone_check`).  Not
    among the reference's options."""
    from .segments import one_of, read_option

    def from_opt(value, who):
        if not isinstance(value, str):
            raise ValueError(f"{who}={value!r}: 'report', 'raise', 'bf16' or None")
        return one_of(N.BACKBONE_CHECKS, "'report', 'raise', 'bf16' or None")(value, who)
    return read_option(opt, "backbone_check", "EAVSR_BACKBONE_CHECK", from_opt, one_of(N.BACKBONE_CHECKS, "report, raise or bf16"))


def wrapper_backbone_check(opt, is_train: bool):
    """`EAVSRPModel.backbone_check`: `backbone_check_option(opt)` outside training; under `isTrain` an `opt.backbone_check` is refused
    and None is returned otherwise -- training reads neither the option nor the environment (`networks.active_backbone_check`
    likewise ignores a mode that only the environment set while gradients are enabled)"""
    if is_train:
        if getattr(opt, "backbone_check", None) is not None:
            raise ValueError("opt.backbone_check: the census belongs to the 16-bit backbone, an inference mode (networks.set_backbone_dtype)")
        return None
    return backbone_check_option(opt)


def cache_dtype_option(opt=None):
    """None, "fp16" or "bf16": what the long-clip path's frame store holds its features in (`EAVSRP.forward_long(cache_dtype=...)`,
    DESIGN 7n) -- `opt.cache_dtype` ("fp16" / "bf16" or torch.float16 / torch.bfloat16), falling back to the environment where the
    options do not carry it (EAVSR_CACHE_DTYPE=fp16|bf16), None -- fp32, today's stores -- where neither does.  Not among the
    reference's options."""
    from .segments import one_of, read_option

    def from_opt(value, who):
        try:
            return FS.check_cache_dtype(value)
        except ValueError:
            raise ValueError(f"{who}={value!r}: 'fp16', 'bf16' (torch.float16 / torch.bfloat16) or None") from None
    return read_option(opt, "cache_dtype", "EAVSR_CACHE_DTYPE", from_opt, one_of(tuple(FS.CACHE_DTYPES), "fp16 or bf16"))


def png_encoder_option(opt=None) -> str:
    """"host" or "device": who encodes the PNG files `harness.super_resolve` writes -- `opt.png_encoder`, falling back to the
    environment where the options do not carry it (EAVSR_PNG_ENCODER=host|device), "host" where neither does.  Not among the
    reference's options."""
    from .segments import one_of, read_option
    return read_option(opt, "png_encoder", "EAVSR_PNG_ENCODER", one_of(("host", "device"), "'host' or 'device'"),
                       one_of(("host", "device"), "host or device"), default="host")


def png_decoder_option(opt=None) -> str:
    """"host" or "device": who undoes the scanline filters of the PNG files `harness.super_resolve` reads -- `opt.png_decoder`,
    falling back to the environment where the options do not carry it (EAVSR_PNG_DECODER=host|device), "host" where neither does.
    Not among the reference's options."""
    from .segments import one_of, read_option
    return read_option(opt, "png_decoder", "EAVSR_PNG_DECODER", one_of(("host", "device"), "'host' or 'device'"),
                       one_of(("host", "device"), "host or device"), default="host")


class EAVSRPModel:
    """Stand-in of EAVSRPModel / EAVSRPx2Model (models/eavsrp_model.py:18-119): set_input / forward / test /
    optimize_parameters / get_current_visuals / load_networks / save_networks with the reference's
    checkpoint format ({'state_dict': ...}, base_model.py:159-217).  One process per GPU; with several
    processes (torch.distributed initialised) the training step averages the loss gradients with one
    bucketed RCCL all-reduce (eavsr_amd.shard.GradientAllReducer) instead of nn.DataParallel.
    From epoch opt.npost on (eavsrp_model.py:85-97) the training forward multiplies the SR output by the validity mask of the HR
    frames warped by a frozen PWC-Net's flow (eavsr_amd.pwc), loaded from opt.pwc_path at the first such forward; PWC-Net gets no
    gradients and is not part of the checkpoint.  The reference also calls netGF there and discards its output (the x4 model
    even fails inside it, eavsrp_model.py:686): it is not computed here."""

    def __init__(self, opt):
        self.opt = opt
        self.scale = opt.scale
        self.isTrain = getattr(opt, "isTrain", False)
        # opt.frame_chunk / opt.cpu_cache (not among the reference's options): the opt-in long-clip inference path (EAVSRP.forward_long)
        self.frame_chunk, self.cpu_cache = long_clip_options(opt)
        # opt.cache_dtype (not among the reference's options): the frame store's features in 16 bits, outside training
        self.cache_dtype = cache_dtype_option(opt)
        if self.isTrain and getattr(opt, "cache_dtype", None) is not None:
            raise ValueError("opt.cache_dtype: the 16-bit feature cache is an inference option (EAVSRP.forward_long); training keeps "
                             "its activations for the backward pass in fp32")
        # opt.cache_check (not among the reference's options): the census of that cache and what is done about it (addendum)
        if self.isTrain and getattr(opt, "cache_check", None) is not None:
            raise ValueError("opt.cache_check: the census belongs to the 16-bit feature cache, an inference option (EAVSRP.forward_long)")
        self.cache_check = cache_check_option(opt)
        if not self.isTrain:      # (training reads neither: an environment set for inference runs does not stop it)
            FS.check_cache_check(self.cache_check, self.cache_dtype)
        # opt.backbone_check (not among the reference's options): the range census of the 16-bit backbone modes (addendum)
        self.backbone_check = wrapper_backbone_check(opt, self.isTrain)
        # opt.out_size (not among the reference's options): the SR frames resized to any target size, outside training
        if self.isTrain and getattr(opt, "out_size", None) is not None:
            raise ValueError("opt.out_size: the resize of the SR frames is an inference option (resize.resize_frames has no backward); "
                             "training compares with the HR frames at the network's own size")
        from .resize import out_size_option
        self.out_size = None if self.isTrain else out_size_option(opt)      # (training reads neither the option nor the environment)
        self.png_encoder = png_encoder_option(opt)
        # opt.pad_frames (not among the reference's options): frames of any size outside training (EAVSRP.forward_long(pad=...))
        from .segments import pad_option
        self.pad_frames = pad_option(opt)
        # opt.tile / opt.tile_overlap (not among the reference's options): frames of any resolution outside training (EAVSRP.forward_tiled)
        from .segments import tile_options, DEFAULT_TILE_OVERLAP
        self.tile, self.tile_overlap = tile_options(opt)
        if self.tile_overlap is None:
            self.tile_overlap = DEFAULT_TILE_OVERLAP
        # opt.ensemble (not among the reference's options): the self-ensemble outside training (EAVSRP.forward_ensemble); None: off
        from .segments import ensemble_options
        self.ensemble = ensemble_options(opt)
        if self.ensemble == (0,):
            self.ensemble = None
        # opt.train_precision (not among the reference's options): the opt-in bf16 training mode (networks.set_train_precision)
        if getattr(opt, "train_precision", None) is not None:
            N.set_train_precision(opt.train_precision)
        # opt.deterministic (not among the reference's options): the opt-in deterministic training mode (networks.set_deterministic)
        if getattr(opt, "deterministic", None) is not None:
            N.set_deterministic(opt.deterministic)
        gpu_ids = list(getattr(opt, "gpu_ids", [0]))
        if len(gpu_ids) == 0:
            raise RuntimeError("eavsr_amd has no CPU path (--gpu_ids -1 is the reference's CPU mode)")
        self.device = torch.device("cuda", gpu_ids[0])
        self.visual_names = ["data_lr_seq", "data_hr_seq", "data_sr_seq"]
        self.loss_names = ["EAVSRP_L1", "EAVSRP_Total"]
        self.model_names = ["EAVSRP"]
        self.netEAVSRP = N.init_net(EAVSRP(opt, getattr(opt, "spynet_pretrained", None)), gpu_ids=gpu_ids)
        self.time, self.isfirst, self.num = 0.0, True, 0
        self.epoch = 0
        self.netPWCNET = None      # loaded at the first training forward with epoch >= opt.npost (_pwc_net)
        self.start_epoch = 0
        self.metric = 0            # learning-rate policy 'plateau' (base_model.py:34)
        self.optimizers, self.schedulers = [], []
        if self.isTrain:
            self.optimizer_EAVSRP = make_optimizer(self.netEAVSRP, opt)
            trainable = [p for p in self.netEAVSRP.parameters() if p.requires_grad]   # what the gradient all-reduce carries
            self.optimizers = [self.optimizer_EAVSRP]
            from .shard import GradientAllReducer
            self.grad_sync = GradientAllReducer(trainable)
            self.netEAVSRP.train()
        self.sync_parameters()

    def sync_parameters(self, src: int = 0) -> int:
        """Several processes (one per GPU): every rank takes rank `src`'s parameters and buffers, once -- at construction and
        after `load_networks` -- so that data-parallel replicas start identical whatever each rank seeded or loaded.  The
        reference gets this from nn.DataParallel's per-forward replication (models/networks.py:67-74); here it is one start-up
        broadcast and nothing per step (eavsr_amd.shard.broadcast_module).  No-op on one process."""
        from .shard import broadcast_module
        return broadcast_module(self.netEAVSRP, src)

    def setup(self, opt=None):
        """base_model.py:56-70, what train_basic.py:42 / test_basic.py call after construction: learning-rate schedulers
        (training), then the checkpoint named by opt.load_iter / opt.load_path and, with opt.load_optimizers, the optimizer
        file."""
        opt = opt if opt is not None else self.opt
        load_iter = getattr(opt, "load_iter", 0)
        if self.isTrain:
            self.schedulers = [get_scheduler(optimizer, opt) for optimizer in self.optimizers]
            for scheduler in self.schedulers:
                scheduler.last_epoch = load_iter
        if (isinstance(load_iter, int) and load_iter > 0) or getattr(opt, "load_path", "") != "":
            self.load_networks(load_iter)
            if getattr(opt, "load_optimizers", False):
                self.load_optimizers(load_iter)
        self.print_networks(getattr(opt, "verbose", False))

    def update_learning_rate(self):
        """base_model.py:131-138"""
        for i, scheduler in enumerate(self.schedulers):
            if scheduler.__class__.__name__ == "ReduceLROnPlateau":
                scheduler.step(getattr(self, "metric", 0))
            else:
                scheduler.step()
            print("lr of %s = %.7f" % (self.optimizer_names[i], scheduler.get_last_lr()[0]))

    def print_networks(self, verbose=False):
        """base_model.py:272-284"""
        print("---------- Networks initialized -------------")
        num_params = sum(p.numel() for p in self.netEAVSRP.parameters())
        if verbose:
            print(self.netEAVSRP)
        print("[Network %s] Total number of parameters : %.3f M" % (self.model_names[0], num_params / 1e6))
        print("-----------------------------------------------")

    def eval(self):
        self.netEAVSRP.eval()

    def train(self):
        self.netEAVSRP.train()

    def set_input(self, input, epoch=0):
        self.data_lr_seq = input["lr_seq"].to(self.device)
        self.data_hr_seq = input["hr_seq"].to(self.device) if "hr_seq" in input else None
        self.image_name = input.get("fname")
        self.idx = min(self.opt.n_frame // 2, self.data_lr_seq.shape[1] - 1)
        self.epoch = epoch

    def forward(self):
        if getattr(self, "backbone_check", None) is not None and N.BACKBONE_CHECK is None and not (self.isTrain and self.netEAVSRP.training):
            # opt.backbone_check: this method once more under the check (a mode set on the module itself stays as it is).  Every call
            # below leads to EAVSRP.forward / forward_long, which count; one entry of `netEAVSRP.backbone_census` per window
            with N.backbone_check(self.backbone_check), torch.no_grad():
                return self.forward()
        if self.isTrain and self.netEAVSRP.training:
            self.data_sr_seq = self.netEAVSRP(self.data_lr_seq)
            self.data_sr = self.data_sr_seq[:, self.idx]
            if self.masked_phase():
                self.data_hr_align, self.mask = self.hr_align_and_mask()
                self.data_sr_seq = self.data_sr_seq * self.mask
            return
        start = time.time()
        long_path = not self.isTrain and (self.frame_chunk is not None or self.cpu_cache)
        cache = "host" if self.cpu_cache else "device"
        if not self.isTrain and self.cache_dtype is not None:
            # the long path on a store that holds its features in 16 bits, with whatever else is set
            with torch.no_grad():
                self.data_sr_seq = self.netEAVSRP.forward_cached(self.data_lr_seq, self.cache_dtype, ensemble=self.ensemble,
                                                                 tile=self.tile, overlap=self.tile_overlap, pad=self.pad_frames,
                                                                 frame_chunk=self.frame_chunk, cache=cache,
                                                                 **_checked(self.cache_check))
        elif not self.isTrain and self.ensemble is not None:
            # the mean over flips / transposes of the frame, tiled and padded as below
            with torch.no_grad():
                self.data_sr_seq = self.netEAVSRP.forward_ensemble(self.data_lr_seq, ensemble=self.ensemble, tile=self.tile,
                                                                   overlap=self.tile_overlap, pad=self.pad_frames,
                                                                   frame_chunk=self.frame_chunk, cache=cache)
        elif not self.isTrain and (self.tile is not None or self.pad_frames is not None):
            # frames of any resolution (overlapped tiles, blended: DESIGN 7j) or of any size
            with torch.no_grad():
                self.data_sr_seq = self.netEAVSRP.forward_video(self.data_lr_seq, tile=self.tile, tile_overlap=self.tile_overlap,
                                                                pad=self.pad_frames, frame_chunk=self.frame_chunk, cache=cache)
        elif long_path:
            with torch.no_grad():
                self.data_sr_seq = self.netEAVSRP.forward_long(self.data_lr_seq, frame_chunk=self.frame_chunk, cache=cache)
        else:
            self.data_sr_seq = self.netEAVSRP(self.data_lr_seq)
        if self.out_size is not None:      # (never under isTrain) what `harness.evaluate` scores and `save_visuals` writes
            from .resize import resize_frames
            self.data_sr_seq = resize_frames(self.data_sr_seq, self.out_size)
        self.data_sr = self.data_sr_seq[:, self.idx]
        end = time.time()
        if not self.isfirst:
            self.time += end - start
            self.num += 1
        self.isfirst = False

    def masked_phase(self) -> bool:
        """epoch >= opt.npost: the training forward masks the SR output (eavsrp_model.py:85)"""
        return self.epoch >= getattr(self.opt, "npost", 350)

    def _pwc_net(self):
        """The frozen PWC-Net, read from opt.pwc_path (default ./pwc/pwc-default, models/pwc_net.py:246) once.  Several
        processes: every rank reads its file and the ranks agree (`shard.all_ranks_ok`) before any of them goes on."""
        if self.netPWCNET is not None:
            return self.netPWCNET
        from . import pwc
        from .shard import all_ranks_ok
        path = getattr(self.opt, "pwc_path", "./pwc/pwc-default")
        net, err = None, None
        try:
            if not os.path.isfile(path):
                raise FileNotFoundError(f"PWC-Net weights {path!r} not found (opt.pwc_path): training at epoch {self.epoch} >= "
                                        f"opt.npost = {getattr(self.opt, 'npost', 350)} masks the loss with PWC-Net's flow")
            net = pwc.load_pwc_weights(pwc.PWCNET(), path).to(self.device).eval()
            for p in net.parameters():
                p.requires_grad_(False)
        except Exception as e:      # noqa: BLE001 -- re-raised below, on every rank
            err = e
        if not all_ranks_ok(err is None):
            if err is not None:
                raise err
            raise RuntimeError("another rank failed to load the PWC-Net weights (opt.pwc_path); aborting on every rank")
        self.netPWCNET = net
        return net

    def hr_align_and_mask(self):
        """(hr_align (n,t,3,H,W), mask (n,t,1,H,W)) of every frame: BaseModel.get_backwarp(lr, hr, PWC-Net, scale)
        (base_model.py:338-354), all n*t frame pairs in one PWC-Net call"""
        from . import pwc
        lr, hr = self.data_lr_seq, self.data_hr_seq
        n, t = lr.shape[:2]
        hr_align, mask = pwc.get_backwarp(lr.reshape((n * t,) + tuple(lr.shape[2:])), hr.reshape((n * t,) + tuple(hr.shape[2:])),
                                          self._pwc_net(), self.scale)
        return hr_align.view((n, t) + tuple(hr_align.shape[1:])), mask.view((n, t) + tuple(mask.shape[1:]))

    def test(self):
        with torch.no_grad():
            self.forward()

    def backward(self):
        # criterionL1(hr, sr).mean()  (eavsrp_model.py:109-113)
        self.loss_EAVSRP_L1 = (self.data_hr_seq - self.data_sr_seq).abs().mean()
        self.loss_EAVSRP_Total = self.loss_EAVSRP_L1
        with AG.grad_sink():         # per-use parameter gradients are summed in place by the wgrad kernels
            self.loss_EAVSRP_Total.backward()
        self.grad_sync.finish()      # one bucketed all-reduce over the loss gradients (no-op on 1 process)

    def optimize_parameters(self):
        self.forward()
        self.optimizer_EAVSRP.zero_grad(set_to_none=True)
        self.backward()
        self.optimizer_EAVSRP.step()

    def get_current_losses(self):
        return {n: float(getattr(self, "loss_" + n).detach()) for n in self.loss_names if hasattr(self, "loss_" + n)}

    def get_current_visuals(self):
        out = {}
        for name in self.visual_names:
            v = getattr(self, name, None)
            if v is not None:
                out[name] = torch.clamp(v.detach() * 255.0, 0, 255).round()
        return out

    # ---- checkpoint and optimizer files (base_model.py:159-270) ---------------------------------
    @property
    def optimizer_names(self):
        return ["EAVSRP_optimizer_%s" % getattr(self.opt, "optimizer", "Adam")]   # eavsrp_model.py:31

    def _save_dir(self):
        d = getattr(self, "save_dir", None) or os.path.join(getattr(self.opt, "checkpoints_dir", "./ckpt"),
                                                             getattr(self.opt, "name", "eavsr"))
        os.makedirs(d, exist_ok=True)
        return d

    def _network_path(self, epoch_or_path):
        """An int is the reference's epoch (`<save_dir>/<name>_model_<epoch>.pth`, base_model.py:161-162); opt.load_path
        overrides it on load (base_model.py:182-183); a string is taken as the file itself."""
        if isinstance(epoch_or_path, int):
            return os.path.join(self._save_dir(), "%s_model_%d.pth" % (self.model_names[0], epoch_or_path))
        return epoch_or_path

    def save_networks(self, epoch_or_path):
        """{'state_dict': cpu tensors} (base_model.py:165-170); with an epoch number the optimizer files are written
        beside it as the reference does (base_model.py:172)."""
        path = self._network_path(epoch_or_path)
        torch.save({"state_dict": {k: v.detach().cpu() for k, v in self.netEAVSRP.state_dict().items()}}, path)
        if isinstance(epoch_or_path, int) and self.isTrain:
            self.save_optimizers(epoch_or_path)
        return path

    def load_networks(self, epoch_or_path):
        """Every key of the file must exist in the network with the same shape and every parameter of the network
        must be in the file: the reference `exit()`s on either mismatch (base_model.py:193-213); here it raises.
        Several processes: a COLLECTIVE -- every rank calls it (as every rank runs train_basic.py / test_basic.py).  The ranks
        first agree that all of them read and checked their file (`shard.all_ranks_ok`): if one failed, every rank raises --
        nobody is left blocked in the parameter broadcast that follows, and that broadcast can never pair with another rank's
        next collective.  Then rank 0's parameters and buffers go to everybody (`sync_parameters`)."""
        from .shard import all_ranks_ok
        path, err = None, None
        try:
            path = self._network_path(epoch_or_path)
            if isinstance(epoch_or_path, int) and getattr(self.opt, "load_path", ""):
                path = self.opt.load_path
            sd = torch.load(path, map_location="cpu")
            sd = sd.get("state_dict", sd)
            own = self.netEAVSRP.state_dict()
            unknown = [k for k in sd if k not in own]
            missing = [k for k in own if k not in sd]
            if unknown:
                raise RuntimeError("Saved parameter named [%s] is not in the network (%d such keys)" % (unknown[0], len(unknown)))
            if missing:
                raise RuntimeError("Parameter named [%s] is not in %s (%d such keys)" % (missing[0], path, len(missing)))
            for k, v in sd.items():
                if tuple(own[k].shape) != tuple(v.shape):
                    raise RuntimeError("While copying the parameter named [%s], whose dimensions in the model are %s and "
                                       "whose dimensions in the checkpoint are %s." % (k, list(own[k].shape), list(v.shape)))
            self.netEAVSRP.load_state_dict(sd, strict=True)
        except Exception as e:      # noqa: BLE001 -- re-raised below, on every rank
            err = e
        if not all_ranks_ok(err is None):
            if err is not None:
                raise err
            raise RuntimeError(f"load_networks({epoch_or_path!r}): another rank failed to load its checkpoint; aborting on every rank")
        self.sync_parameters()
        if isinstance(epoch_or_path, int):
            self.start_epoch = epoch_or_path
        return path

    def save_optimizers(self, epoch):
        """One file per optimizer: {'name', 'epoch', 'state_dict'} at <save_dir>/<optimizer name>.pth (base_model.py:251-260)."""
        assert len(self.optimizers) == len(self.optimizer_names)
        for name, optimizer in zip(self.optimizer_names, self.optimizers):
            torch.save({"name": name, "epoch": epoch, "state_dict": optimizer.state_dict()},
                       os.path.join(self._save_dir(), name + ".pth"))

    def load_optimizers(self, epoch):
        """base_model.py:262-270: name and epoch recorded in the file must match."""
        assert len(self.optimizers) == len(self.optimizer_names)
        for name, optimizer in zip(self.optimizer_names, self.optimizers):
            state = torch.load(os.path.join(self._save_dir(), name + ".pth"), map_location=self.device)
            if state["name"] != name or state["epoch"] != epoch:
                raise RuntimeError("optimizer file %s.pth holds (%s, epoch %s), expected (%s, epoch %s)"
                                   % (name, state["name"], state["epoch"], name, epoch))
            optimizer.load_state_dict(state["state_dict"])
