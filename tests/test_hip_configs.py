"""GPU parity / property tests at the sizes BASELINE.json names (`pytest -m gpu`).

configs[1]  eavsrp x4, 7 x 3 x 180 x 320 fp32          -- one full-size clip against the CPU oracle (<= 1e-3 max abs, the
            north star's bound), in the DEFAULT kernel mode, asserting that the kernels the bench times really ran.
configs[2]  eavsrpx2, 8 clips x 7 x 3 x 256 x 256 bf16 -- full size: one clip against the CPU oracle (fp32 <= 1e-3; bf16 by PSNR
            against the oracle), the batch 16-bit vs fp32 by PSNR.
configs[3]  eavsrp x4 training step, 2 x 7 x 3 x 96 x 96 -- full size: the loss is finite and decreases.
configs[4]  eavsrp x4, 15 x 3 x 540 x 960 fp16          -- the 15-frame recurrence and the x4 + fp16 backbone against the
            oracle at a size the CPU affords (1 x 15 x 3 x 64 x 96), and the full-size clip as a property test.
configs[0] (1 x 7 x 3 x 64 x 64) is tests/test_hip_model.py::test_end_to_end_golden.

The oracle forwards take ~1 min (full 180 x 320 clip) / ~15 s (15 x 64 x 96) on the GPU box's host cores.
"""
from argparse import Namespace

import pytest
import torch

from oracle import eavsr_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _net(cuda, tag="x4", preset="trained_like", n_frame=7):
    from eavsr_amd.eavsrp_model import EAVSRP
    net = EAVSRP(Namespace(predict=False, n_frame=n_frame, n_flow=5, scale=4 if tag == "x4" else 2), None)
    sd = H.filled(H.model_shapes(tag), preset)
    net.load_state_dict(sd, strict=True)
    return net.to(cuda).eval(), sd


def _clip(n, t, h, w, seed):
    from eavsr_amd.utils.synthetic import synthetic_clip
    return synthetic_clip(n, t, h, w, seed=seed)


# ---------------------------------------------------------------------------------------------------------- configs[1]
def test_config1_full_size_clip_matches_the_cpu_oracle(cuda):
    """BASELINE.json configs[1] / the north star's parity statement: one 7 x 3 x 180 x 320 clip, fp32, default kernel
    mode (Winograd F(4x4,3x3) 3x3 convolutions, bf16x6 predictor heads and SPyNet 7x7 layers, fused DCNv2), against the CPU oracle's
    `eavsrp_forward` (models/eavsrp_model.py:202-240) within 1e-3 max abs.  The 64 x 64 golden clip is too small for the
    Winograd kernels to engage; this is the size the bench times."""
    from eavsr_amd import ops
    assert ops.CONV_MODE == "winograd4" and ops.DCN_MODE == "il6" and ops.CONV5_MODE == "bf16x6" and ops.CONV7_MODE == "bf16x6"
    net, sd = _net(cuda)
    clip = _clip(1, 7, 180, 320, seed=0)
    caps = []
    hook = net.reconstruction.register_forward_pre_hook(lambda m, inp: caps.append(inp[0]))
    with torch.no_grad():
        with ops.profile() as prof:
            y = net(clip.to(cuda))
        hook.remove()
        names = set(prof.summary())
        y = y.cpu()
        # the sub-batch shape the bench launches (2 clips) must give the same per-clip answer
        y2 = net(torch.cat([clip, _clip(1, 7, 180, 320, seed=1)], 0).to(cuda))[0:1].cpu()
        # ... and so must exactly what bench.py times: 4 clips as two 2-clip HIP graphs on two streams (clip 3 = this clip)
        from eavsr_amd.graph import StreamedForward
        four = torch.cat([_clip(1, 7, 180, 320, seed=2), _clip(1, 7, 180, 320, seed=3), _clip(1, 7, 180, 320, seed=1), clip], 0).to(cuda)
        sf = StreamedForward(net, four, groups=2)
        y4 = sf(four)[3:4].cpu()
        del sf, four
        ref, ref_feats = O.eavsrp_forward(sd, clip, 4, return_feats=True)
    assert tuple(y.shape) == (1, 7, 3, 720, 1280)
    ran = {"conv3x3_64to64_wino4", "conv5x5_64to120_x6", "conv7x7_32to64_x6", "conv7x7_64to32_x6", "conv7x7_8to32_x6", "conv7x7_16to2_x6"}
    assert ran <= names, names
    assert {"dcnv2_il_heads", "flow_warp_pair", "flow_warp"} <= names, names
    err = H.maxabs(y, ref)
    assert err <= 1e-3, err
    assert H.maxabs(y2, ref) <= 1e-3
    assert H.maxabs(y4, ref) <= 1e-3, H.maxabs(y4, ref)
    assert O.psnr_255(y, ref) >= 80.0      # on clamp * 255 * round images (util/util.py:302-320)
    # The output is dominated by the bilinear skip of the LR frames (the network adds ~ +-0.04 on a [0, 1] image), so 1e-3 on it is a
    # loose statement about alignment and propagation.  The sensitive one: the propagated branch features --
    # the inputs of `reconstruction` (eavsrp_model.py:229-240) -- at THIS size and in THIS kernel mode, <= 1e-3 of their scale.
    n, t = 1, 7
    srcs = caps[0]      # five frame-major tensors (t * n, 64, h, w): spatial, backward_1, forward_1, backward_2, forward_2
    worst = 0.0
    for src, key in zip(srcs, ["spatial", "backward_1", "forward_1", "backward_2", "forward_2"]):
        got = src.view(t, n, 64, 180, 320).cpu()
        want = torch.stack([ref_feats[key][i] for i in range(t)], 0)
        scale = max(1.0, want.abs().max().item())
        e = H.maxabs(got, want) / scale
        worst = max(worst, e)
        assert e <= 1e-3, (key, e)
    print(f"configs[1] 1x7x3x180x320: max|hip - oracle| = {err:.3e}, PSNR = {O.psnr_255(y, ref):.1f} dB; branch features "
          f"(inputs of reconstruction) worst max|hip - oracle| / scale = {worst:.3e}; 4-clip StreamedForward clip 3: {H.maxabs(y4, ref):.3e}")


def test_config1_dcnv2_launch_shape_properties(cuda):
    """The DCNv2 launch of configs[1] at full size (2 x 64 x 180 x 320, dg = 8; 460 tiles on 256 workgroups, both kernels of the
    alignment's hot path) through size-independent properties: zero offsets + unit masks == conv2d; integer offsets shift the taps;
    linearity in the sampled features; the round-4 schedule agrees with round 2's to re-association; heads mode == the explicit
    form of the same offsets / masks."""
    import torch.nn.functional as F
    from eavsr_amd import ops
    from tests.golden import cases
    n, c, h, w, D = 2, 64, 180, 320, 8
    x = cases.randn(301, n, c, h, w)
    x2 = cases.randn(302, n, c, h, w)
    wt = cases.randn(303, 64, c, 3, 3, scale=1.0 / (c * 9) ** 0.5)
    b = cases.randn(304, 64, scale=0.1)
    gx, gx2, gw, gb = x.to(cuda), x2.to(cuda), wt.to(cuda), b.to(cuda)
    xil, xil2 = ops.to_il8(gx), ops.to_il8(gx2)
    zero_off = torch.zeros(n, 18 * D, h, w, device=cuda)
    ones = torch.ones(n, 9 * D, h, w, device=cuda)
    prev = ops.DCN_IL_IMPL
    try:
        for impl in ("il2", "il"):
            ops.set_dcn_il_impl(impl)
            y0 = ops.dcnv2_il(xil, zero_off, ones, gw, gb, D).cpu()
            assert H.maxabs(y0, F.conv2d(x, wt, b, 1, 1)) <= 3e-5, impl
        ops.set_dcn_il_impl("il2")
        # integer offsets (+1, -2) for every tap == the conv of the shifted, zero-extended image
        off = zero_off.clone()
        off[:, 0::2] = 1.0
        off[:, 1::2] = -2.0
        ys = ops.dcnv2_il(xil, off, ones, gw, gb, D).cpu()
        xs = torch.zeros(n, c, h + 8, w + 8)
        xs[:, :, 4:-4, 4:-4] = x
        ref = F.conv2d(xs, wt, b, 1, 1)[:, :, 5:5 + h, 2:2 + w]
        assert H.maxabs(ys, ref) <= 3e-5
        # linearity in the sampled features (bias removed), with sub-pixel offsets and random masks
        offr = (cases.randn(305, n, 18 * D, h, w, scale=0.8)).to(cuda)
        mk = cases.rand(306, n, 9 * D, h, w).to(cuda)
        ya = ops.dcnv2_il(xil, offr, mk, gw, None, D)
        yb = ops.dcnv2_il(xil2, offr, mk, gw, None, D)
        yab = ops.dcnv2_il(ops.to_il8(gx * 2.0 - gx2 * 0.5), offr, mk, gw, None, D)
        sc = max(1.0, yab.abs().max().item())
        assert H.maxabs(yab.cpu(), (2.0 * ya - 0.5 * yb).cpu()) <= 2e-5 * sc
        # round 4 against round 2 on the same inputs
        ops.set_dcn_il_impl("il")
        ya_r2 = ops.dcnv2_il(xil, offr, mk, gw, None, D)
        assert H.maxabs(ya.cpu(), ya_r2.cpu()) <= 1e-5 * sc
        # heads mode (affine expansion + sigmoid inside) == explicit mode on the expanded offsets / masks
        ops.set_dcn_il_impl("il2")
        heads = torch.cat([cases.randn(307, n, 4 * D, h, w, scale=0.2) + torch.tensor([1.0, 0, 0, 1.0]).repeat(D).view(1, 4 * D, 1, 1),
                           cases.randn(308, n, 2 * D, h, w, scale=0.8), cases.randn(309, n, 9 * D, h, w, scale=2.0)], 1)
        offe = O.affine_offsets(heads[:, :4 * D], heads[:, 4 * D:6 * D], D)
        yh = ops.dcnv2_il(xil, heads.to(cuda), None, gw, gb, D, heads=True)
        ye = ops.dcnv2_il(xil, offe.to(cuda), torch.sigmoid(heads[:, 6 * D:]).to(cuda), gw, gb, D)
        assert H.maxabs(yh.cpu(), ye.cpu()) <= 2e-5 * max(1.0, ye.abs().max().item())
    finally:
        ops.set_dcn_il_impl(prev)


def _outside_window_fraction(off, D, h, w):
    """fraction of (pixel, group, tap) samples of explicit offsets (n, 18 D, h, w) with a bilinear corner outside dcnv2_il2's LDS
    window (8 x 32 tile; rows y0 - 6 .. y0 + 13, columns x0 - 8 .. x0 + 39: csrc/dcnv2_il2.hip), and outside the IMAGE (a sample
    the validity gate -1 < p < size drops)"""
    n = off.shape[0]
    o = off.view(n, D, 9, 2, h, w)
    ky = torch.tensor([-1., -1., -1., 0., 0., 0., 1., 1., 1.]).view(1, 1, 9, 1, 1)
    kx = torch.tensor([-1., 0., 1., -1., 0., 1., -1., 0., 1.]).view(1, 1, 9, 1, 1)
    ys = torch.arange(h).view(1, 1, 1, h, 1)
    xs = torch.arange(w).view(1, 1, 1, 1, w)
    py, px = ys + ky + o[:, :, :, 0], xs + kx + o[:, :, :, 1]
    ry = 6 + (ys % 8) + ky + torch.floor(o[:, :, :, 0])
    rx = 8 + (xs % 32) + kx + torch.floor(o[:, :, :, 1])
    outside = (ry < 0) | (ry > 18) | (rx < 0) | (rx > 46)
    invalid = (py <= -1) | (py >= h) | (px <= -1) | (px >= w)
    return outside.float().mean().item(), invalid.float().mean().item()


def test_config1_dcnv2_launch_shape_out_of_window_samples_match_the_oracle(cuda):
    """the RARE path of `dcnv2_il2` (samples whose corners leave the LDS window are served inline from global
    memory) at the bench's own launch -- 2 x 64 x 180 x 320, 460 tiles walked by 256 persistent workgroups -- against the CPU oracle
    (`O.dcnv2`, the mmcv op as networks.py:627-630 consumes it), in the explicit and in the heads form, with sigma = 8 px offsets:
    a stated, non-zero fraction of the samples leaves the window and another leaves the image."""
    from eavsr_amd import ops
    from tests.golden import cases
    assert ops.DCN_IL_IMPL == "il2"
    n, c, h, w, D = 2, 64, 180, 320, 8
    x = cases.randn(401, n, c, h, w)
    wt = cases.randn(402, 64, c, 3, 3, scale=1.0 / (c * 9) ** 0.5)
    b = cases.randn(403, 64, scale=0.1)
    xil = ops.to_il8(x.to(cuda))
    # explicit offsets / masks (mmcv's signature)
    off = cases.randn(404, n, 18 * D, h, w, scale=8.0)
    off[:, :, :3, :] -= 6.0            # a band at the top / left that pushes samples out of the image as well
    off[:, 1::2, :, -4:] += 9.0
    mask = cases.rand(405, n, 9 * D, h, w)
    f_out, f_inv = _outside_window_fraction(off, D, h, w)
    assert f_out > 0.2 and f_inv > 0.005, (f_out, f_inv)
    with ops.profile() as prof:
        y = ops.dcnv2_il(xil, off.to(cuda), mask.to(cuda), wt.to(cuda), b.to(cuda), D).cpu()
    assert "dcnv2_il" in set(prof.summary()), set(prof.summary())
    ref = O.dcnv2(x, off, mask, wt, b, 1, 1, 1, 1, D)
    sc = max(1.0, ref.abs().max().item())
    err_e = H.maxabs(y, ref) / sc
    assert err_e <= 3e-5, err_e
    # heads form (AdaptBlockOffset's 15 D channels; networks.py:298-315), translations of sigma = 8 px
    heads = torch.cat([cases.randn(406, n, 4 * D, h, w, scale=0.3) + torch.tensor([1.0, 0, 0, 1.0]).repeat(D).view(1, 4 * D, 1, 1),
                       cases.randn(407, n, 2 * D, h, w, scale=8.0), cases.randn(408, n, 9 * D, h, w, scale=2.0)], 1)
    offh = O.affine_offsets(heads[:, :4 * D], heads[:, 4 * D:6 * D], D)
    fh_out, fh_inv = _outside_window_fraction(offh, D, h, w)
    st = ops.dcn_offset_stats(heads.to(cuda), D)
    assert fh_out > 0.2 and fh_inv > 0.001 and abs(st["frac_outside_lds_window"] - fh_out) < 1e-3, (fh_out, fh_inv, st)
    with ops.profile() as prof:
        yh = ops.dcnv2_il(xil, heads.to(cuda), None, wt.to(cuda), b.to(cuda), D, heads=True).cpu()
    assert "dcnv2_il_heads" in set(prof.summary()), set(prof.summary())
    refh = O.dcnv2(x, offh, torch.sigmoid(heads[:, 6 * D:]), wt, b, 1, 1, 1, 1, D)
    err_h = H.maxabs(yh, refh) / max(1.0, refh.abs().max().item())
    assert err_h <= 3e-5, err_h
    print(f"dcnv2_il2 at 2x64x180x320, sigma = 8 px: explicit {f_out:.3f} of the samples outside the LDS window, {f_inv:.4f} outside "
          f"the image, max|hip - oracle| / scale = {err_e:.2e}; heads {fh_out:.3f} / {fh_inv:.4f}, {err_h:.2e}")


# ---------------------------------------------------------------------------------------------------------- configs[4]
def test_config4_fifteen_frame_recurrence_matches_the_cpu_oracle_fp32_and_fp16(cuda):
    """t = 15 bidirectional propagation (configs[4]'s recurrence depth; eavsrp_model.py:242-329 index maps for t > n_frame)
    on the x4 model: exact fp32 against the oracle <= 1e-3, then the fp16 backbone against the SAME oracle output by PSNR
    (BASELINE.json: reduced precision is judged by PSNR vs the CPU reference)."""
    from eavsr_amd import networks as Nw
    net, sd = _net(cuda)
    clip = _clip(1, 15, 64, 96, seed=11)
    with torch.no_grad():
        y = net(clip.to(cuda)).cpu()
        ref = O.eavsrp_forward(sd, clip, 4)
        assert tuple(y.shape) == (1, 15, 3, 256, 384)
        err = H.maxabs(y, ref)
        assert err <= 1e-3, err
        psnrs = {}
        for dt in ("fp16", "bf16"):
            try:
                Nw.set_backbone_dtype(dt)
                y16 = net(clip.to(cuda)).cpu()
            finally:
                Nw.set_backbone_dtype(None)
            assert torch.isfinite(y16).all()
            psnrs[dt] = O.psnr_255(y16, ref)
    assert psnrs["fp16"] >= 60.0 and psnrs["bf16"] >= 50.0, psnrs
    print(f"configs[4] recurrence 1x15x3x64x96: fp32 max err {err:.3e}; PSNR vs oracle fp16 {psnrs['fp16']:.1f} dB, "
          f"bf16 {psnrs['bf16']:.1f} dB")


def test_config4_mid_size_fp16_backbone_psnr_against_the_cpu_oracle(cuda):
    """configs[4]'s reduced-precision claim against the REFERENCE arithmetic at a size where the 16-bit kernels
    run as they do at 540 x 960 (several tiles per persistent workgroup, the Winograd / bf16x6 routes of the fp32 remainder):
    1 x 15 x 3 x 128 x 192, fp16 backbone PSNR vs `O.eavsrp_forward` (models/eavsrp_model.py:202-240), fp32 within 1e-3 of it."""
    from eavsr_amd import networks as Nw, ops
    net, sd = _net(cuda)
    clip = _clip(1, 15, 128, 192, seed=21)
    with torch.no_grad():
        y32 = net(clip.to(cuda)).cpu()
        try:
            Nw.set_backbone_dtype("fp16")
            with ops.profile() as prof16:
                y16 = net(clip.to(cuda)).cpu()
        finally:
            Nw.set_backbone_dtype(None)
        names16 = set(prof16.summary())
        ref = O.eavsrp_forward(sd, clip, 4)
    assert tuple(y16.shape) == (1, 15, 3, 512, 768) and torch.isfinite(y16).all()
    assert {"conv3x3_64to64_h16", "dcnv2_il16_heads"} <= names16, names16
    err = H.maxabs(y32, ref)
    assert err <= 1e-3, err
    psnr16, psnr32 = O.psnr_255(y16, ref), O.psnr_255(y32, ref)
    assert psnr32 >= 80.0 and psnr16 >= 60.0, (psnr32, psnr16)
    print(f"configs[4] mid size 1x15x3x128x192: fp32 max|hip - oracle| = {err:.3e} ({psnr32:.1f} dB); fp16 backbone vs the oracle {psnr16:.1f} dB")


def test_config4_full_size_long_sequence_fp16(cuda):
    """BASELINE.json configs[4] at full size, 1 x 15 x 3 x 540 x 960 -> 2160 x 3840: too large for the CPU oracle, so
    size-independent properties: finite output of the right shape, the fp16-backbone forward within 60 dB PSNR of the
    exact fp32 forward of the same kernels, peak HBM logged (it must fit one 288 GB MI355X with room to spare).

    The fp16-versus-fp32 comparison shares the encoder, the glue and the tail between its two sides, so an offset that wraps in
    them (the tail's 15 x 256 x 540 x 960 tensor is 7.96 GB, past 2^32 bytes) would pass it.  The independent anchor: the encoder
    and `EAVSRP.upsample` run once more on all 15 full-size frames, and frames 0 and 14 are compared with the CPU oracle, by the
    method and under the bound of tests/test_hip_model.py::test_encoder_and_upsampling_tail_vs_oracle (seeded branch features,
    1e-4 max(1, |ref|max)).  Not on a 64 x 96 crop: the reconstruction backbone's channel attention averages over the whole plane,
    so a crop of the full-size result is not the result of the crop; the oracle instead does the two frames at the full 540 x 960,
    one frame at a time, which it affords."""
    from eavsr_amd import networks as Nw
    from eavsr_amd import ops
    net, sd = _net(cuda)
    clip = _clip(1, 15, 540, 960, seed=4).to(cuda)
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        y32 = net(clip)
        peak32 = torch.cuda.max_memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        try:
            Nw.set_backbone_dtype("fp16")
            y16 = net(clip)
        finally:
            Nw.set_backbone_dtype(None)
        peak16 = torch.cuda.max_memory_allocated()
        assert tuple(y16.shape) == (1, 15, 3, 2160, 3840)
        assert torch.isfinite(y32).all() and torch.isfinite(y16).all()
        # PSNR on the GPU (the frames are 1.5 GB): clamp * 255 * round as util/util.py:302-320
        q = lambda v: torch.clamp(v * 255.0, 0, 255).round()
        mse = (q(y16) - q(y32)).div(255.0).pow(2).mean().item()
        psnr = float("inf") if mse == 0 else -10.0 * torch.log10(torch.tensor(mse)).item()
        maxd = (y16 - y32).abs().max().item()
    assert psnr >= 60.0, psnr
    assert peak32 < 200 * 2 ** 30, peak32
    print(f"configs[4] 1x15x3x540x960: fp16-vs-fp32 PSNR {psnr:.1f} dB, max diff {maxd:.2e}; peak HBM fp32 "
          f"{peak32 / 2 ** 30:.1f} GiB, fp16 backbone {peak16 / 2 ** 30:.1f} GiB")
    del y16, y32
    torch.cuda.empty_cache()
    x = clip[0]                                                  # (15, 3, 540, 960): n = 1, frame-major
    with torch.no_grad():
        f = net.encoder(x)
    for i in (0, 14):
        ref_f = O.encoder(sd, "encoder.", x[i:i + 1].cpu())
        err = H.maxabs(f[i:i + 1].cpu(), ref_f)
        print(f"configs[4] full size, encoder frame {i}: max|hip - oracle| = {err:.3e} (|ref|max {ref_f.abs().max().item():.3f})")
        assert err <= 1e-4 * max(1.0, ref_f.abs().max().item()), (i, err)
    del f
    g = torch.Generator(device=cuda).manual_seed(44)
    names = ["spatial", "backward_1", "forward_1", "backward_2", "forward_2"]
    feats = {k: [torch.randn(1, 64, 540, 960, device=cuda, generator=g) * 0.5 for _ in range(15)] for k in names}
    with torch.no_grad(), ops.profile() as prof:
        y = net.upsample(clip, feats)
    ran = set(prof.summary())
    assert tuple(y.shape) == (1, 15, 3, 2160, 3840)
    assert "conv3x3_64to256_wino4" in ran and "conv3x3_320to64_wino4" in ran, ran
    for i in (0, 14):
        ref = O.upsample(sd, clip[:, i:i + 1].cpu(), {k: [v[i].cpu()] for k, v in feats.items()}, 4)
        err = H.maxabs(y[:, i:i + 1].cpu(), ref)
        print(f"configs[4] full size, tail frame {i}: max|hip - oracle| = {err:.3e} (|ref|max {ref.abs().max().item():.3f})")
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (i, err)


# ---------------------------------------------------------------------------------------------------------- configs[2]
def test_config2_x2_model_full_size_bf16(cuda):
    """BASELINE.json configs[2]: eavsrpx2, 8 clips x 7 x 3 x 256 x 256.  Pinned to the reference at FULL resolution (VERDICT r4
    item 4): clip 5 of the batch through the CPU oracle's `eavsrp_forward(sd, clip, 2)` (models/eavsrpx2_model.py:124-365, ~20 s of
    host time) -- the HIP fp32 forward in the default kernel mode within 1e-3 max abs of it (with the kernels the bench times
    asserted), and the bf16-backbone output quoted by PSNR against that ORACLE output, not against our own fp32 forward."""
    from eavsr_amd import networks as Nw, ops
    assert ops.CONV_MODE == "winograd4" and ops.DCN_MODE == "il6" and ops.CONV5_MODE == "bf16x6" and ops.CONV7_MODE == "bf16x6"
    net, sd = _net(cuda, "x2")
    clip_cpu = _clip(8, 7, 256, 256, seed=2)
    clip = clip_cpu.to(cuda)
    with torch.no_grad():
        with ops.profile() as prof:
            y32 = net(clip)
        names32 = set(prof.summary())
        try:
            Nw.set_backbone_dtype("bf16")
            with ops.profile() as prof16:
                y16 = net(clip)
            names16 = set(prof16.summary())
        finally:
            Nw.set_backbone_dtype(None)
        ref5 = O.eavsrp_forward(sd, clip_cpu[5:6], 2)
    assert tuple(y16.shape) == (8, 7, 3, 512, 512) and tuple(ref5.shape) == (1, 7, 3, 512, 512)
    assert torch.isfinite(y32).all() and torch.isfinite(y16).all()
    assert {"conv3x3_64to64_wino4", "conv5x5_64to120_x6", "dcnv2_il_heads", "flow_warp_pair"} <= names32, names32
    assert {"conv3x3_64to64_h16", "dcnv2_il16_heads"} <= names16, names16
    err = H.maxabs(y32[5:6].cpu(), ref5)
    assert err <= 1e-3, err                       # the north star's fp32 bound, at the size and in the mode the bench runs
    psnr32 = O.psnr_255(y32[5:6].cpu(), ref5)
    psnr16 = O.psnr_255(y16[5:6].cpu(), ref5)     # bf16 backbone against the REFERENCE arithmetic
    assert psnr32 >= 80.0, psnr32
    assert psnr16 >= 50.0, psnr16
    psnr = O.psnr_255(y16.cpu(), y32.cpu())       # the whole batch, 16-bit against fp32 (what bench.py's psnr_vs_fp32 reports)
    assert psnr >= 50.0, psnr
    # clips are independent: clip 5 of the batch equals clip 5 on its own (fp32)
    with torch.no_grad():
        one = net(clip[5:6])
    assert H.maxabs(one.cpu(), y32[5:6].cpu()) <= 1e-5
    print(f"configs[2] x2 8x7x3x256x256: clip 5 fp32 max|hip - oracle| = {err:.3e} (PSNR {psnr32:.1f} dB); bf16 backbone vs the oracle "
          f"{psnr16:.1f} dB, vs our fp32 forward over the batch {psnr:.1f} dB")


# ---------------------------------------------------------------------------------------------------------- configs[3]
def test_config3_training_step_full_size_loss_decreases(cuda):
    """BASELINE.json configs[3] on one GPU: 2 clips x 7 x 3 x 96 x 96, HR 384 x 384, L1, Adam with the reference's two
    groups -- the loss is finite on every step and lower after a few steps on the same batch (gradient parity itself is
    tests/test_hip_backward.py, at the size the CPU autograd oracle affords)."""
    from eavsr_amd.eavsrp_model import EAVSRPModel
    opt = Namespace(predict=False, n_frame=7, n_flow=5, scale=4, isTrain=True, gpu_ids=[0], lr=1e-4, beta1=0.9,
                    beta2=0.999, weight_decay=0.0, npost=350)
    model = EAVSRPModel(opt)
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    lr = _clip(2, 7, 96, 96, seed=7)
    hr = torch.nn.functional.interpolate(lr.view(14, 3, 96, 96), scale_factor=4, mode="bicubic",
                                         align_corners=False).clamp(0, 1).view(2, 7, 3, 384, 384)
    model.set_input({"lr_seq": lr, "hr_seq": hr, "fname": "synthetic"}, epoch=0)
    losses = []
    for _ in range(6):
        model.optimize_parameters()
        losses.append(model.get_current_losses()["EAVSRP_L1"])
    assert all(l == l and l < 1e3 for l in losses), losses
    assert losses[-1] < losses[0], losses
    print(f"configs[3] 2x7x3x96x96 training step: L1 {losses[0]:.5f} -> {losses[-1]:.5f}")


def _host_mem_available_gib():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / 2 ** 20
    except OSError:
        pass
    return 0.0


def test_config3_gradients_at_the_bench_shape_match_oracle_autograd(cuda):
    """configs[3]'s gradients at the size the bench trains at (7 x 3 x 96 x 96 crops, HR 384 x 384; both clips
    of the per-GPU batch when the host has the ~26 GB CPU autograd needs, one otherwise), against CPU autograd through the
    oracle (models/eavsrp_model.py:109-119: L1 loss, backward), asserting that the routes that carry the bench's training step --
    the crop-sized bf16x6 3x3 convolution `conv3x3_64to64_x6s` and the bf16x6 3x3 weight gradient (`eavsr_wgrad3_mode() == 1`
    behind `conv_wgrad3x3`) -- are the ones that ran."""
    from eavsr_amd import ops, autograd as AG
    from eavsr_amd.eavsrp_model import EAVSRP
    from tests.test_hip_backward import _oracle_forward_with_grad
    nclips = 2 if _host_mem_available_gib() >= 48.0 else 1
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda).train()
    clip = _clip(nclips, 7, 96, 96, seed=7)
    hr = torch.nn.functional.interpolate(clip.view(-1, 3, 96, 96), scale_factor=4, mode="bicubic",
                                         align_corners=False).clamp(0, 1).view(nclips, 7, 3, 384, 384)
    with ops.profile() as prof:
        with AG.grad_sink():
            out = net(clip.to(cuda))
            loss = (out - hr.to(cuda)).abs().mean()
            loss.backward()
    names = set(prof.summary())
    assert {"conv3x3_64to64_x6s", "conv_wgrad3x3", "conv_wgrad5x5", "conv_wgrad1x1"} <= names, names
    # round 6: DCNv2's backward runs on the sampler's side (csrc/dcn_bwd.hip) -- no column tensor, no im2col / col2im launches
    assert "dcnv2_bwd" in names and not ({"dcnv2_im2col", "dcnv2_col2im"} & names), names
    assert ops.lib().eavsr_wgrad3_mode() == 1
    # round 6 (late): consecutive RCABs hand the plane sums `sum_hw d r` over -- they leave the epilogue of the next block's last
    # input-gradient convolution (desc.sum_mul); only a group's LAST block (its d comes from the group's closing convolution) still
    # launches them
    summ = prof.summary()
    assert summ["plane_sum"]["calls"] * 10 <= summ["rcab_tail_bwd"]["calls"], (summ["plane_sum"]["calls"], summ["rcab_tail_bwd"]["calls"])
    watch = ["conv_last.weight", "backbone.forward_2.main.2.rg.3.res.0.weight", "backbone.backward_1.main.2.rg.29.res.2.weight",
             "backbone.forward_1.main.2.rg.30.weight", "backbone.backward_2.main.0.weight", "fusion.backward_1.weight",
             "deform_align.forward_1.weight", "deform_align.backward_2.adastn.mask_conv.bias",
             "deform_align.backward_1.adastn.transform_matrix_conv.weight", "deform_align.forward_1.flow_l2.concat.0.weight",
             "deform_align.forward_2.trans_l1.conv_first.weight", "encoder.tail.bias", "upsample1.0.weight",
             "backbone.backward_1.main.2.rg.7.ca.conv_du.0.weight", "backbone.forward_2.main.2.rg.0.res.0.bias"]
    csd = {k: (v.clone().requires_grad_(True) if k in watch else v) for k, v in sd.items()}
    with torch.enable_grad():
        with torch.no_grad():
            flows = O.compute_flow(sd, clip)
        out_c = _oracle_forward_with_grad(csd, clip, flows)
        loss_c = (out_c - hr).abs().mean()
    gs = torch.autograd.grad(loss_c, [csd[k] for k in watch])
    assert abs(loss.item() - loss_c.item()) <= 1e-4, (loss.item(), loss_c.item())
    params = dict(net.named_parameters())
    worst = ("", 0.0)
    for k, gc in zip(watch, gs):
        gg = params[k].grad
        assert gg is not None, k
        scale = max(1e-7, gc.abs().max().item())
        e = H.maxabs(gg.cpu(), gc) / scale
        worst = max(worst, (k, e), key=lambda p: p[1])
        assert e <= 5e-3, (k, e, scale)
    print(f"configs[3] gradients at {nclips} x 7 x 3 x 96 x 96 vs oracle autograd: loss {loss.item():.6f} / {loss_c.item():.6f}, "
          f"worst relative gradient error {worst[1]:.2e} ({worst[0]}) over {len(watch)} parameters")
