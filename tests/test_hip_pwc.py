"""PWC-Net of the late-training validity mask on the GPU (csrc/pwc.hip, eavsr_amd/pwc.py): every entry point against CPU torch
or the restatement (tests/pwc_ref.py), PWCNET / get_backwarp against the reference's fixtures, and the training step from
epoch opt.npost on, eager and graphed."""
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

from oracle import eavsr_oracle as O
from tests import helpers as H
from tests import pwc_ref
from tests.test_pwc_host import CASES, load_case, pwc_weights

pytestmark = pytest.mark.gpu


def _slice_of(t, dev, before=3, after=5, batch_pad=0):
    """t as a channel slice of a larger NCHW buffer on `dev` (a batch stride beyond c*h*w)"""
    n, c, h, w = t.shape
    buf = torch.full((n + batch_pad, before + c + after, h, w), float("nan"), device=dev)
    view = buf[:n, before:before + c]
    view.copy_(t)
    return view


# (n, cin, h, w, cout, stride, dilation): every layer shape of the extractor / decoder / refiner at the two crop sizes' levels
CONV_SHAPES = [
    (4, 3, 64, 64, 16, 2, 1), (4, 16, 32, 32, 16, 1, 1), (4, 16, 32, 32, 32, 2, 1), (4, 32, 16, 16, 64, 2, 1),
    (4, 64, 7, 9, 96, 2, 1), (4, 96, 5, 5, 128, 2, 1), (4, 128, 3, 3, 196, 2, 1), (4, 196, 1, 1, 196, 1, 1),
    (2, 117, 16, 16, 128, 1, 1), (2, 245, 16, 16, 128, 1, 1), (2, 373, 16, 16, 96, 1, 1), (2, 469, 16, 16, 64, 1, 1),
    (2, 533, 16, 16, 32, 1, 1), (2, 565, 16, 16, 2, 1, 1), (2, 661, 2, 2, 2, 1, 1), (3, 81, 1, 1, 128, 1, 1),
    (2, 565, 32, 32, 128, 1, 1), (2, 128, 32, 32, 128, 1, 2), (2, 128, 32, 32, 128, 1, 4), (2, 128, 16, 16, 96, 1, 8),
    (2, 96, 16, 16, 64, 1, 16), (2, 96, 2, 2, 64, 1, 16), (2, 96, 1, 1, 64, 1, 16), (2, 64, 16, 16, 32, 1, 1),
    (2, 32, 16, 16, 2, 1, 1),
]


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pwc_conv3x3_against_torch(cuda, shape):
    from eavsr_amd import ops
    n, cin, h, w, cout, stride, dil = shape
    g = torch.Generator().manual_seed(hash(shape) % 1000)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    for act in ("lrelu", None):
        ref = F.conv2d(x, wt, b, stride=stride, padding=dil, dilation=dil)
        if act:
            ref = F.leaky_relu(ref, 0.1)
        got = ops.pwc_conv3x3(x.to(cuda), wt.to(cuda), b.to(cuda), stride=stride, dilation=dil, act=act).cpu()
        assert got.shape == ref.shape
        assert H.maxabs(got, ref) <= 2e-5 * max(1.0, ref.abs().max().item()), (act, H.maxabs(got, ref))
    # channel slices with a batch stride in and out; nothing outside the output slice is written
    xs = _slice_of(x, cuda)
    out_buf = torch.full((n, cout + 7, ref.shape[2], ref.shape[3]), 123.0, device=cuda)
    ops.pwc_conv3x3(xs, wt.to(cuda), b.to(cuda), stride=stride, dilation=dil, act=None, out=out_buf[:, 4:4 + cout])
    ob = out_buf.cpu()
    assert H.maxabs(ob[:, 4:4 + cout], ref) <= 2e-5 * max(1.0, ref.abs().max().item())
    assert bool((ob[:, :4] == 123.0).all()) and bool((ob[:, 4 + cout:] == 123.0).all())


@pytest.mark.parametrize("cin,h,w", [(2, 1, 1), (2, 4, 4), (529, 1, 1), (661, 2, 2), (629, 4, 4), (597, 8, 8), (597, 16, 16),
                                     (2, 7, 5)])
def test_pwc_deconv4x4s2_against_torch(cuda, cin, h, w):
    from eavsr_amd import ops
    g = torch.Generator().manual_seed(cin + h)
    n = 3
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cin, 2, 4, 4, generator=g) / (4 * cin) ** 0.5
    b = torch.randn(2, generator=g)
    ref = F.conv_transpose2d(x, wt, b, stride=2, padding=1)
    got = ops.pwc_deconv4x4s2(_slice_of(x, cuda), wt.to(cuda), b.to(cuda)).cpu()
    assert H.maxabs(got, ref) <= 2e-5 * max(1.0, ref.abs().max().item())
    out_buf = torch.zeros(n, 9, 2 * h, 2 * w, device=cuda)
    ops.pwc_deconv4x4s2(x.to(cuda), wt.to(cuda), b.to(cuda), out=out_buf[:, 3:5])
    assert H.maxabs(out_buf[:, 3:5].cpu(), ref) <= 2e-5 * max(1.0, ref.abs().max().item())
    assert float(out_buf[:, :3].abs().max()) == 0 and float(out_buf[:, 5:].abs().max()) == 0


@pytest.mark.parametrize("c,h,w", [(32, 32, 32), (64, 16, 16), (96, 8, 8), (128, 4, 4), (196, 2, 2), (196, 1, 1), (32, 9, 18)])
def test_pwc_correlation_against_restatement(cuda, c, h, w):
    from eavsr_amd import ops
    g = torch.Generator().manual_seed(c * h)
    a, b = torch.randn(3, c, h, w, generator=g), torch.randn(3, c, h, w, generator=g)
    ref = F.leaky_relu(pwc_ref.correlation(a, b), 0.1)
    out_buf = torch.zeros(3, 81 + 10, h, w, device=cuda)
    ops.pwc_correlation(_slice_of(a, cuda), _slice_of(b, cuda, 1, 0), out=out_buf[:, 6:87])
    assert H.maxabs(out_buf[:, 6:87].cpu(), ref) <= 1e-5 * max(1.0, ref.abs().max().item())
    assert float(out_buf[:, :6].abs().max()) == 0 and float(out_buf[:, 87:].abs().max()) == 0


def _check_warp(got, mask_got, x, flow_full, tol=1e-5):
    out = pwc_ref.grid_warp(x, flow_full)
    ones = out[:, -1:]
    mask = pwc_ref.threshold(ones)
    exempt = (ones - 0.999).abs() <= 1e-5
    agree = (mask == mask_got) | exempt
    assert bool(agree.all()), int((~agree).sum())
    sure = (~exempt).expand_as(got)
    assert H.maxabs(got[sure], (out[:, :-1] * mask)[sure]) <= tol
    return mask


@pytest.mark.parametrize("level,h,w", [(5, 2, 2), (4, 4, 4), (3, 8, 8), (2, 32, 32), (3, 9, 22)])
def test_pwc_backwarp_decoder_mode(cuda, level, h, w):
    from eavsr_amd import ops
    g = torch.Generator().manual_seed(level * 7 + h)
    c = pwc_ref.CH[level - 1]
    x = torch.randn(2, c, h, w, generator=g)
    flow = torch.randn(2, 2, h, w, generator=g) * 0.6
    flt = pwc_ref.FLT_BACKWARP[level]
    got = ops.pwc_backwarp(_slice_of(x, cuda), _slice_of(flow, cuda, 7, 2), flt).cpu()
    _, mask_got = ops.pwc_backwarp(x.to(cuda), flow.to(cuda), flt, with_mask=True)
    mask = _check_warp(got, mask_got.cpu(), x, flow * flt)
    assert 0 < float(mask.mean()) < 1


@pytest.mark.parametrize("scale,h,w", [(4, 9, 11), (2, 16, 16)])
def test_pwc_backwarp_final_mode(cuda, scale, h, w):
    from eavsr_amd import ops
    g = torch.Generator().manual_seed(scale * 31 + h)
    hr = torch.rand(2, 3, h * scale, w * scale, generator=g)
    flow = torch.randn(2, 2, h, w, generator=g) * 1.5
    got, mask_got = ops.pwc_backwarp(hr.to(cuda), flow.to(cuda), float(scale), with_mask=True)
    up = F.interpolate(flow, scale_factor=scale, mode="nearest") * scale
    mask = _check_warp(got.cpu(), mask_got.cpu(), hr, up)
    assert 0 < float(mask.mean()) < 1


def _net(cuda, sd=None):
    from eavsr_amd.pwc import PWCNET
    net = PWCNET()
    net.load_state_dict(sd if sd is not None else pwc_weights(), strict=True)
    return net.to(cuda).eval()


@pytest.mark.parametrize("name", CASES)
def test_pwcnet_and_get_backwarp_against_reference_fixtures(cuda, name):
    from eavsr_amd import ops, pwc
    lr, hr, scale, z = load_case(name)
    net = _net(cuda)
    lr_g, hr_g = lr.to(cuda), hr.to(cuda)
    with torch.no_grad():
        small = ops.resize_bilinear_ac(hr_g, (hr.shape[2] // scale, hr.shape[3] // scale))
        flow = pwc.estimate(lr_g, small, net).cpu()
    assert H.maxabs(flow, torch.from_numpy(z["flow"])) <= 1e-3
    hr_align, mask = pwc.get_backwarp(lr_g, hr_g, net, scale)
    hr_align, mask = hr_align.cpu(), mask.cpu()
    ones = torch.from_numpy(z["ones"])
    # exempt: pixels whose fixture ones channel lies within 5e-4 of the threshold (a fully covered pixel is exactly 1.0, 1e-3 away)
    exempt = (ones - 0.999).abs() <= 5e-4
    assert float(exempt.float().mean()) < 0.01
    want = torch.from_numpy(z["mask"]).float()
    assert bool(((mask == want) | exempt).all())
    assert 0 < float(mask.mean()) < 1
    agree = (mask == want).expand_as(hr_align)
    assert H.maxabs(hr_align[agree], torch.from_numpy(z["hr_align"]).float()[agree]) <= 1e-3


def test_get_backwarp_runs_only_the_hip_kernels(cuda):
    from eavsr_amd import ops, pwc
    lr, hr, scale, _ = load_case("x4_72x88")
    net = _net(cuda)
    lr_g, hr_g = lr.to(cuda), hr.to(cuda)
    pwc.get_backwarp(lr_g, hr_g, net, scale)
    torch.cuda.synchronize()
    with ops.profile() as prof:
        pwc.get_backwarp(lr_g, hr_g, net, scale)
    names = set(prof.summary())
    assert {"pwc_conv3x3", "pwc_deconv4x4s2", "pwc_correlation", "pwc_backwarp", "resize_bilinear", "resize_bilinear_ac"} <= names
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as tp:
        pwc.get_backwarp(lr_g, hr_g, net, scale)
        torch.cuda.synchronize()
    ops_seen = {e.name for e in tp.events()}
    banned = [o for o in ops_seen if o in ("aten::convolution", "aten::conv2d", "aten::conv_transpose2d", "aten::grid_sampler_2d",
                                           "aten::cat") or o.startswith("aten::upsample")]
    assert not banned, banned
    with pytest.raises(RuntimeError):
        pwc.get_backwarp(lr, hr, net, scale)          # CPU tensors: no CPU path


def _opt(scale, tmp_path, npost=350):
    return Namespace(predict=False, n_frame=3, n_flow=5, scale=scale, isTrain=True, gpu_ids=[0], lr=1e-4, beta1=0.9,
                     beta2=0.999, weight_decay=0.0, npost=npost, load_path="", pwc_path=str(tmp_path / "pwc-default"))


def _write_pwc_file(tmp_path):
    torch.save({k.replace("net", "module"): v for k, v in pwc_weights().items()}, str(tmp_path / "pwc-default"))


@pytest.mark.parametrize("scale", [4, 2])
def test_training_step_at_npost_masks_the_loss(cuda, tmp_path, scale):
    from eavsr_amd.eavsrp_model import EAVSRPModel
    from eavsr_amd.eavsrpx2_model import EAVSRPx2Model
    from eavsr_amd.utils.synthetic import synthetic_clip
    cls = EAVSRPModel if scale == 4 else EAVSRPx2Model
    model = cls(_opt(scale, tmp_path))            # constructs with no PWC-Net file present
    sd = H.filled(H.model_shapes("x4" if scale == 4 else "x2"), "trained_like")
    model.netEAVSRP.load_state_dict(sd, strict=True)
    lr_hw = 64
    clip = synthetic_clip(1, 3, lr_hw, lr_hw, seed=11)
    hr = synthetic_clip(1, 3, lr_hw * scale, lr_hw * scale, seed=12)
    model.set_input({"lr_seq": clip, "hr_seq": hr, "fname": "x"}, epoch=350)
    with pytest.raises(FileNotFoundError, match="pwc_path"):
        model.optimize_parameters()
    _write_pwc_file(tmp_path)
    model.set_input({"lr_seq": clip, "hr_seq": hr, "fname": "x"}, epoch=350)
    model.forward()
    mask = model.mask.detach().cpu()
    assert tuple(mask.shape) == (1, 3, 1, lr_hw * scale, lr_hw * scale)
    assert tuple(model.data_hr_align.shape) == (1, 3, 3, lr_hw * scale, lr_hw * scale)
    assert 0 < float(mask.mean()) <= 1 and set(mask.unique().tolist()) <= {0.0, 1.0}
    assert model.model_names == ["EAVSRP"] and all(not p.requires_grad for p in model.netPWCNET.parameters())
    model.optimizer_EAVSRP.zero_grad(set_to_none=True)
    model.backward()
    loss = model.loss_EAVSRP_L1.item()
    if scale == 2:
        with torch.no_grad():
            ref = O.eavsrp_forward(sd, clip, 2)
        loss_c = ((hr - ref * mask).abs().mean()).item()
        assert abs(loss - loss_c) <= 1e-4
        return
    from tests.test_hip_backward import _oracle_forward_with_grad
    watch = ["conv_last.weight", "backbone.forward_2.main.2.rg.3.res.0.weight", "fusion.backward_1.weight",
             "deform_align.forward_1.weight", "encoder.tail.bias"]
    csd = {k: (v.clone().requires_grad_(True) if k in watch else v) for k, v in sd.items()}
    with torch.enable_grad():
        with torch.no_grad():
            flows = O.compute_flow(sd, clip)
        out_c = _oracle_forward_with_grad(csd, clip, flows)
        loss_c = (hr - out_c * mask).abs().mean()
    gs = torch.autograd.grad(loss_c, [csd[k] for k in watch])
    assert abs(loss - loss_c.item()) <= 1e-4
    params = dict(model.netEAVSRP.named_parameters())
    for k, gc in zip(watch, gs):
        scale_g = max(1e-7, gc.abs().max().item())
        assert H.maxabs(params[k].grad.cpu(), gc) <= 5e-3 * scale_g, (k, H.maxabs(params[k].grad.cpu(), gc), scale_g)
    assert "netPWCNET" not in "".join(model.netEAVSRP.state_dict())


def test_graphed_step_recaptures_at_npost(cuda, tmp_path):
    from eavsr_amd.eavsrp_model import EAVSRPModel
    from eavsr_amd.graph import GraphedTrainStep
    from eavsr_amd.utils.synthetic import synthetic_clip
    _write_pwc_file(tmp_path)
    model = EAVSRPModel(_opt(4, tmp_path, npost=5))
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    data = {"lr_seq": synthetic_clip(1, 3, 64, 64, seed=1), "hr_seq": synthetic_clip(1, 3, 256, 256, seed=2), "fname": "x"}
    model.set_input(data, epoch=4)
    step = GraphedTrainStep(model, warmup=1)
    assert not step.masked
    try:
        step.step(data, epoch=4)
        # the eager losses of the current parameters, unmasked and masked
        with torch.no_grad():
            model.epoch = 4
            model.forward()
            plain = (model.data_hr_seq - model.data_sr_seq).abs().mean().item()
            model.epoch = 5
            model.forward()
            masked = (model.data_hr_seq - model.data_sr_seq).abs().mean().item()
        assert masked != plain
        step.step(data, epoch=5)                 # crossing npost: one recapture, then the masked loss
        assert step.masked
        assert abs(model.loss_EAVSRP_L1.item() - masked) <= 1e-5 * max(1.0, masked)
        g0 = step.graph
        with torch.no_grad():
            model.forward()
            eager = (model.data_hr_seq - model.data_sr_seq).abs().mean().item()
        step.step(data, epoch=6)                 # same phase: no recapture
        assert step.graph is g0
        assert abs(model.loss_EAVSRP_L1.item() - eager) <= 1e-5 * max(1.0, eager)
    finally:
        step.close()
