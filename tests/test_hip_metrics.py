"""The fused per-frame PSNR / SSIM kernel (csrc/metrics.hip) against the host restatements: integer torch arithmetic and
`harness.calc_psnr` / `harness.calc_ssim` evaluated on CPU tensors (float64 SSIM), never against the kernel's own output.

Bounds.  sse and the 8-bit frame are integers: equality.  PSNR against `calc_psnr`, which averages in fp32: 1e-4 dB.  SSIM: the
kernel and `calc_ssim` both carry the moments in fp64 and differ in summation order only, which moves the frame's mean by about
1e-13 (the same definition with one 121-tap window instead of 11 + 11 taps differs by <= 2.6e-13 on the bright, nearly flat image,
the worst content here); the bound is 1e-9, four orders below what fp32 moments give on that image (1.7e-5 .. 4.7e-5), so an fp32
kernel fails.  Identical frames: |ssim - 1| <= 1e-12 and psnr == inf.  (On an MI355X the largest SSIM difference over all cases
is 1.6e-13, on the 11 x 11 bright-flat frame.)"""
import math
import os
from argparse import Namespace

import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 11, 11), (2, 3, 37, 53), (3, 1, 64, 96), (2, 3, 180, 320), (7, 3, 720, 1280)]
CONTENTS = ["noise", "bright_flat", "ramp", "identical", "out_of_range", "half_to_even"]
SSIM_TOL = 1e-9
PSNR_TOL_DB = 1e-4


def make_pair(content, shape, seed):
    """(sr, hr, scale) CPU fp32 tensors of `shape` = (F, C, H, W)"""
    g = torch.Generator().manual_seed(seed)
    f, c, h, w = shape
    noise = lambda: torch.randn(shape, generator=g) * (4.0 / 255.0)
    if content == "noise":
        hr = torch.rand(shape, generator=g)
        return hr + noise(), hr, 255.0
    if content == "bright_flat":       # filt(x^2) - filt(x)^2 cancels at magnitude 65 025
        hr = (250 + torch.randint(0, 6, shape, generator=g)).float() / 255.0
        return hr + noise(), hr, 255.0
    if content == "ramp":
        hr = torch.linspace(0.0, 1.0, w).view(1, 1, 1, w).expand(shape).contiguous()
        return hr + noise(), hr, 255.0
    if content == "identical":
        hr = torch.rand(shape, generator=g)
        return hr.clone(), hr, 255.0
    if content == "out_of_range":      # both images reach outside [0, 1]: the clamp
        hr = torch.rand(shape, generator=g) * 1.6 - 0.3
        return hr + noise() * 8, hr, 255.0
    if content == "half_to_even":      # scale 1, every sample exactly k + 0.5 (k = -1 and 255 included: the clamp comes first)
        sr = torch.randint(-1, 256, shape, generator=g).float() + 0.5
        hr = torch.randint(-1, 256, shape, generator=g).float() + 0.5
        return sr, hr, 1.0
    raise ValueError(content)


def quantised(v, scale):
    return torch.clamp(v * scale, 0, 255).round()      # get_current_visuals, on the CPU


def check_against_host(sr, hr, scale, sse, ssim, rgb8, label):
    """sse (F,) int64, ssim (F,) float64, rgb8 (F, H, W, C) uint8: the kernel's results, already on the CPU"""
    from eavsr_amd import harness
    f, c, h, w = sr.shape
    q_sr, q_hr = quantised(sr, scale), quantised(hr, scale)
    want_sse = ((q_sr.long() - q_hr.long()) ** 2).sum(dim=(1, 2, 3))
    print(f"{label}: sse {sse.tolist()} want {want_sse.tolist()}")
    assert sse.dtype == torch.int64 and torch.equal(sse, want_sse)
    assert rgb8.dtype == torch.uint8 and torch.equal(rgb8, q_sr.to(torch.uint8).permute(0, 2, 3, 1).contiguous())
    assert ssim.dtype == torch.float64
    for i in range(f):
        psnr = harness.psnr_from_sse(int(sse[i]), c * h * w)
        e = int(want_sse[i])
        want_psnr = math.inf if e == 0 else -10.0 * math.log10(e / (c * h * w) / 255.0 ** 2)
        host_psnr = harness.calc_psnr(q_sr[i], q_hr[i])
        host_ssim = harness.calc_ssim(q_sr[i], q_hr[i])
        print(f"{label} frame {i}: psnr {psnr!r} float64 {want_psnr!r} calc_psnr {host_psnr!r}; ssim {float(ssim[i])!r} calc_ssim "
              f"{host_ssim!r} diff {abs(float(ssim[i]) - host_ssim):.3e}")
        if e == 0:
            assert psnr == math.inf and host_psnr == math.inf
        else:
            assert psnr == want_psnr
            assert abs(psnr - host_psnr) <= PSNR_TOL_DB
        assert abs(float(ssim[i]) - host_ssim) <= SSIM_TOL


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frame_metrics_against_host_float64(cuda, shape, content):
    from eavsr_amd import ops
    sr, hr, scale = make_pair(content, shape, seed=100 + SHAPES.index(shape) * 10 + CONTENTS.index(content))
    d_sr, d_hr = sr.to(cuda), hr.to(cuda)
    sse, ssim, rgb8 = ops.frame_metrics(d_sr, d_hr, scale=scale, rgb8=True)
    assert sse.is_cuda and ssim.is_cuda and rgb8.is_cuda and tuple(rgb8.shape) == (shape[0], shape[2], shape[3], shape[1])
    check_against_host(sr, hr, scale, sse.cpu(), ssim.cpu(), rgb8.cpu(), f"{shape} {content}")
    if content == "identical":
        assert torch.equal(sse.cpu(), torch.zeros(shape[0], dtype=torch.int64))
        assert (ssim.cpu() - 1.0).abs().max().item() <= 1e-12
    # two calls on the same input: bit for bit
    sse2, ssim2, rgb82 = ops.frame_metrics(d_sr, d_hr, scale=scale, rgb8=True)
    assert torch.equal(sse, sse2) and torch.equal(ssim, ssim2) and torch.equal(rgb8, rgb82)
    # without the 8-bit frame the numbers are the same, and the stand-alone quantiser writes the same bytes
    sse3, ssim3, none = ops.frame_metrics(d_sr, d_hr, scale=scale)
    assert none is None and torch.equal(sse, sse3) and torch.equal(ssim, ssim3)
    assert torch.equal(ops.rgb8(d_sr, scale=scale), rgb8)


def test_half_to_even_is_pinned(cuda):
    """0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, ..., 254.5 -> 254, 255.5 -> 255 (clamped first), -0.5 -> 0"""
    from eavsr_amd import ops
    k = torch.arange(-1, 256).float()
    sr = (k + 0.5).repeat(2)[: 22 * 22].view(1, 1, 22, 22).contiguous()
    want = torch.clamp(sr, 0, 255).round()
    assert want.flatten()[:6].tolist() == [0.0, 0.0, 2.0, 2.0, 4.0, 4.0]
    got = ops.rgb8(sr.to(cuda), scale=1.0).cpu()
    assert torch.equal(got.view(1, 1, 22, 22), want.to(torch.uint8))
    sse, ssim, img = ops.frame_metrics(sr.to(cuda), want.to(cuda), scale=1.0, rgb8=True)
    assert int(sse[0]) == 0 and torch.equal(img.cpu(), got)


def test_harness_frame_metrics_n_t_order(cuda):
    from eavsr_amd import harness
    g = torch.Generator().manual_seed(7)
    hr = torch.rand(2, 3, 3, 40, 56, generator=g)
    sr = hr + torch.randn(hr.shape, generator=g) * (4.0 / 255.0)
    got = harness.frame_metrics(sr.to(cuda), hr.to(cuda))
    assert len(got["psnr"]) == 6 and len(got["ssim"]) == 6
    q_sr, q_hr = quantised(sr, 255.0), quantised(hr, 255.0)
    for b in range(2):
        for i in range(3):
            assert abs(got["psnr"][b * 3 + i] - harness.calc_psnr(q_sr[b, i], q_hr[b, i])) <= PSNR_TOL_DB
            assert abs(got["ssim"][b * 3 + i] - harness.calc_ssim(q_sr[b, i], q_hr[b, i])) <= SSIM_TOL
    # tensors that already are visuals: scale 1
    again = harness.frame_metrics(q_sr.to(cuda), q_hr.to(cuda), scale=1.0)
    assert again == got


def test_evaluate_per_frame_report_and_png_files(cuda, tmp_path):
    from eavsr_amd import harness, ops
    from eavsr_amd.eavsrp_model import EAVSRPModel
    from eavsr_amd.utils.synthetic import synthetic_clip
    ops.lib()
    opt = Namespace(predict=False, n_frame=3, n_flow=5, scale=4, isTrain=True, gpu_ids=[0], lr=1e-4, beta1=0.9, beta2=0.999,
                    weight_decay=0.0, npost=350, checkpoints_dir=str(tmp_path), name="run", optimizer="Adam", load_path="")
    model = EAVSRPModel(opt)
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    # two scenes of unequal length: two items of scene 000, one of scene 001
    items = []
    for k, scene in enumerate(["000", "000", "001"]):
        items.append({"lr_seq": synthetic_clip(1, 3, 64, 64, seed=10 + k), "hr_seq": synthetic_clip(1, 3, 256, 256, seed=20 + k),
                      "fname": [["%s_%05d.png" % (scene, 3 * k + i)] for i in range(3)]})
    root = str(tmp_path / "out")
    rep = harness.evaluate(model, items, per_frame=True, calc_ssim_flag=True, save_root=root)

    # the host restatement: every frame of get_current_visuals() on its own, on CPU tensors
    names, want_psnr, want_ssim, want_q, item_psnr, item_ssim = [], [], [], [], [], []
    model.eval()
    for data in items:
        model.set_input(data, 0)
        model.test()
        vis = {k: v.cpu() for k, v in model.get_current_visuals().items()}
        item_psnr.append(harness.calc_psnr(vis["data_sr_seq"], vis["data_hr_seq"]))
        item_ssim.append(harness.calc_ssim(vis["data_sr_seq"], vis["data_hr_seq"]))
        for i in range(3):
            names.append(data["fname"][i][0])
            want_psnr.append(harness.calc_psnr(vis["data_sr_seq"][0, i], vis["data_hr_seq"][0, i]))
            want_ssim.append(harness.calc_ssim(vis["data_sr_seq"][0, i], vis["data_hr_seq"][0, i]))
            want_q.append(vis["data_sr_seq"][0, i].to(torch.uint8))
    assert rep["frame_names"] == names and len(rep["frame_psnr"]) == 9 and len(rep["frame_ssim"]) == 9
    for i in range(9):
        print(f"frame {names[i]}: psnr {rep['frame_psnr'][i]!r} / {want_psnr[i]!r}  ssim {rep['frame_ssim'][i]!r} / {want_ssim[i]!r}")
        assert abs(rep["frame_psnr"][i] - want_psnr[i]) <= PSNR_TOL_DB
        assert abs(rep["frame_ssim"][i] - want_ssim[i]) <= SSIM_TOL
    # the per-item values keep their meaning
    for k in range(3):
        assert abs(rep["psnr"][k] - item_psnr[k]) <= PSNR_TOL_DB and abs(rep["ssim"][k] - item_ssim[k]) <= SSIM_TOL
    want = harness.scene_report(names, want_psnr, want_ssim)
    assert list(rep["report"]["scenes"]) == ["000", "001"]
    assert rep["report"]["scenes"]["000"]["frames"] == 6 and rep["report"]["scenes"]["001"]["frames"] == 3
    assert abs(rep["report"]["final"]["psnr"] - want["final"]["psnr"]) <= PSNR_TOL_DB
    assert abs(rep["report"]["final"]["ssim"] - want["final"]["ssim"]) <= SSIM_TOL
    # the PNG files hold the quantised frames
    assert len(rep["written"]) == 9
    for i, path in enumerate(rep["written"]):
        assert path == os.path.join(root, "sr_patch_0", names[i][:3], names[i][-9:])
        assert torch.equal(harness.read_png(path), want_q[i])
    # ... and are the files the float path writes
    old = harness.evaluate(model, items, calc_ssim_flag=True, save_root=str(tmp_path / "old"))
    for a, b in zip(rep["written"], old["written"]):
        assert open(a, "rb").read() == open(b, "rb").read()
    # the default call returns what it always returned
    assert set(old) == {"psnr", "psnr_mean", "ssim", "ssim_mean", "written", "seconds", "frames", "frames_per_s"}
    assert set(rep) == set(old) | {"frame_psnr", "frame_ssim", "frame_names", "report"}
    assert old["psnr"] == item_psnr or all(abs(a - b) < 1e-6 for a, b in zip(old["psnr"], item_psnr))
