"""The LPIPS (AlexNet) kernels (csrc/lpips.hip) and `eavsr_amd.lpips.LPIPSAlex` against the float64 restatement of the published
definition (tests/lpips_ref.py) on synthetic trained-like weights -- never against the `lpips` package, which does not exist where
these tests run, and never against the kernels' own output.

Bounds.  Nobody had measured an fp32 LPIPS error here, so none is invented: every case also evaluates the restatement in float32
on the CPU, and the kernels (fp32 MFMA, K <= 3 456 terms in another order than the CPU's) must stay within
    |gpu - ref64| <= max(8 |ref32 - ref64|, 2^-20 |ref64|)
per frame (the floor is a few fp32 ulps; the 8 covers a lucky fp32 sample), and for a layer's features within the same form on the
layer's max-abs: max|gpu - ref64| <= max(8 max|ref32 - ref64|, 2^-20 max|ref64|), no element excluded.  On top, from the report's
own precision (three decimals): every per-frame error < 5e-4.  The max-pool is compared for equality.

Measured on an MI355X (profiles/r11_lpips_parity.json has every case): see DESIGN.md section 7.
"""
import json
import os
from argparse import Namespace

import pytest
import torch

from tests import helpers as H
from tests import lpips_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
CAP = 5e-4


def _record(case, **figures):
    """print the measured figures; EAVSR_LPIPS_PARITY_JSON=<file> also collects them there (one JSON object per line)"""
    print(f"{case}: " + "  ".join(f"{k} {v!r}" for k, v in figures.items()))
    path = os.environ.get("EAVSR_LPIPS_PARITY_JSON")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, **figures}) + "\n")


@pytest.fixture(scope="module")
def net(cuda):
    from eavsr_amd.lpips import LPIPSAlex
    n = LPIPSAlex()
    n.load_state_dict(R.synthetic_weights(0), strict=True)
    return n.to(cuda)


def check_features(case, got, ref64, ref32):
    """got: the kernel's fp32 tensor (on the CPU); ref64 / ref32 the restatement's in the two precisions"""
    assert got.dtype == torch.float32 and got.shape == ref64.shape, (got.shape, ref64.shape)
    err_gpu = (got.double() - ref64).abs().max().item()
    err_32 = (ref32.double() - ref64).abs().max().item()
    top = ref64.abs().max().item()
    _record(case, err_gpu=err_gpu, err_ref32=err_32, max_abs=top, bound=max(8 * err_32, FLOOR * top))
    assert torch.isfinite(got).all()
    assert err_gpu <= max(8 * err_32, FLOOR * top)


def check_frames(case, got, ref64, ref32):
    assert got.dtype == torch.float64 and got.shape == ref64.shape, (got.shape, ref64.shape)
    err_gpu = (got - ref64).abs()
    err_32 = (ref32.double() - ref64).abs()
    bound = torch.maximum(8 * err_32, FLOOR * ref64.abs())
    _record(case, value=ref64.tolist(), err_gpu=err_gpu.tolist(), err_ref32=err_32.tolist(), bound=bound.tolist())
    assert torch.isfinite(got).all()
    assert (err_gpu <= bound).all()
    assert (err_gpu < CAP).all()


@pytest.mark.parametrize("size", [(97, 131), (96, 128)], ids=lambda s: "x".join(map(str, s)))
def test_every_kernel_against_the_restatement_layer_by_layer(cuda, net, size):
    """each kernel on its own: the input of layer k is the float64 chain's output of layer k - 1, rounded to fp32, so that a
    difference belongs to the kernel under test"""
    from eavsr_amd import ops
    sd = R.synthetic_weights(0)
    f = 2
    sr, hr = R.image_pair(f, *size, seed=11)
    both = torch.cat([sr, hr])
    convs, lins = net.convs(), net.lins()
    # the first convolution with the front end in it
    got1 = ops.lpips_conv1(sr.to(cuda), hr.to(cuda), convs[0].weight, convs[0].bias, net.scaling_layer.shift, net.scaling_layer.scale)
    ref = {dt: R.layer(R.front_end(both, sd, 255.0, dt), sd, 0) for dt in (torch.float64, torch.float32)}
    check_features(f"{size} conv1+front", got1.cpu(), ref[torch.float64], ref[torch.float32])
    # ... and on visuals with scale 1: the same bits
    vis1 = ops.lpips_conv1(R.quantise(sr, 255.0).to(cuda), R.quantise(hr, 255.0).to(cuda), convs[0].weight, convs[0].bias,
                           net.scaling_layer.shift, net.scaling_layer.scale, scale=1.0)
    assert torch.equal(vis1, got1)
    chain = R.features(both, sd)      # float64
    for k in range(5):
        x = chain[k].float()          # the tap's input, rounded once
        got = ops.lpips_tap(x.to(cuda), lins[k].weight).cpu()
        lin = sd[f"lin{k}.model.1.weight"]
        check_frames(f"{size} tap{k + 1}", got, R.tap_distance(x[:f].double(), x[f:].double(), lin),
                     R.tap_distance(x[:f], x[f:], lin))
        if k == 4:
            break
        if R.LAYERS[k + 1][6]:
            pooled = ops.lpips_maxpool(x.to(cuda)).cpu()
            assert torch.equal(pooled, torch.nn.functional.max_pool2d(x, 3, 2))
            _record(f"{size} maxpool{k + 1}", equal=True, shape=list(pooled.shape))
            x = pooled
        got = ops.lpips_conv(x.to(cuda), convs[k + 1].weight, convs[k + 1].bias).cpu()
        key = R.LAYERS[k + 1][0]
        conv = lambda t: torch.relu(torch.nn.functional.conv2d(t, sd[key + ".weight"].to(t.dtype), sd[key + ".bias"].to(t.dtype),
                                                               padding=R.LAYERS[k + 1][3] // 2))
        check_features(f"{size} conv{k + 2}", got, conv(x.double()), conv(x))


E2E = [(1, 31, 31), (2, 97, 131), (14, 180, 320), (1, 720, 1280)]


@pytest.mark.parametrize("shape", E2E, ids=lambda s: "x".join(map(str, s)))
def test_per_frame_lpips_end_to_end(cuda, net, shape):
    f, h, w = shape
    sd = R.synthetic_weights(0)
    sr, hr = R.image_pair(f, h, w, seed=20 + E2E.index(shape))
    lead = (2, 7) if f == 14 else (f,)
    d_sr, d_hr = sr.to(cuda).view(*lead, 3, h, w), hr.to(cuda).view(*lead, 3, h, w)
    got = net(d_sr, d_hr)                                   # scale 255 on [0, 1] tensors
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == lead
    ref64 = R.lpips(sr, hr, sd)
    ref32 = R.lpips(sr, hr, sd, dtype=torch.float32)
    check_frames(f"e2e {shape}", got.cpu().reshape(-1), ref64, ref32)
    assert (ref64 > 1e-3).all()                             # the pairs differ by something the report would print
    # scale 1 on get_current_visuals() tensors: the same bits
    vis = net(R.quantise(sr, 255.0).to(cuda).view(*lead, 3, h, w), R.quantise(hr, 255.0).to(cuda).view(*lead, 3, h, w), scale=1.0)
    assert torch.equal(vis, got)
    # two calls agree bit for bit; (n, t, ..) input equals the flattened call
    assert torch.equal(net(d_sr, d_hr), got)
    assert torch.equal(net(d_sr.reshape(-1, 3, h, w), d_hr.reshape(-1, 3, h, w)), got.reshape(-1))
    # identical sequences: exactly 0 for every frame
    assert torch.equal(net(d_hr, d_hr.clone()), torch.zeros(lead, dtype=torch.float64, device=cuda))


def test_small_frames_and_bad_tensors_are_refused(cuda, net):
    from eavsr_amd import ops
    with pytest.raises(ValueError, match="31"):
        net(torch.zeros(1, 3, 30, 40, device=cuda), torch.zeros(1, 3, 30, 40, device=cuda))
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 40, 40, device=cuda), torch.zeros(1, 3, 40, 41, device=cuda))
    c, lin, sl = net.convs(), net.lins(), net.scaling_layer
    x = torch.zeros(2, 3, 40, 48, device=cuda)
    feat = torch.zeros(2, 64, 12, 16, device=cuda)
    # CPU tensors
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lpips_conv1(x.cpu(), x.cpu(), c[0].weight, c[0].bias, sl.shift, sl.scale)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lpips_conv(feat.cpu(), c[1].weight, c[1].bias)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lpips_maxpool(feat.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lpips_tap(feat.cpu(), lin[0].weight)
    # non-contiguous tensors
    xt, ft = x.transpose(2, 3), feat.transpose(2, 3)
    assert not xt.is_contiguous() and not ft.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        ops.lpips_conv1(xt, xt, c[0].weight, c[0].bias, sl.shift, sl.scale)
    with pytest.raises(ValueError, match="contiguous"):
        ops.lpips_conv(ft, c[1].weight, c[1].bias)
    with pytest.raises(ValueError, match="contiguous"):
        ops.lpips_maxpool(ft)
    with pytest.raises(ValueError, match="contiguous"):
        ops.lpips_tap(ft, lin[0].weight)
    # shapes the kernels do not take: an argument error from the library (-2), not a launch
    with pytest.raises(RuntimeError, match="argument error -2"):
        ops.lpips_maxpool(torch.zeros(1, 4, 2, 9, device=cuda))
    with pytest.raises(RuntimeError, match="argument error -2"):
        ops.lpips_conv(torch.zeros(1, 24, 8, 8, device=cuda), torch.zeros(64, 24, 3, 3, device=cuda), torch.zeros(64, device=cuda))
    with pytest.raises(RuntimeError, match="argument error -2"):
        ops.lpips_conv1(torch.zeros(1, 3, 6, 40, device=cuda), torch.zeros(1, 3, 6, 40, device=cuda), c[0].weight, c[0].bias, sl.shift,
                        sl.scale)
    # the packed weights live in a registered cache
    from eavsr_amd import graph
    assert len(ops._lpips_pack_cache) >= 1
    graph.clear_weight_caches()
    assert len(ops._lpips_pack_cache) == 0


def test_evaluate_adds_the_third_column(cuda, net, tmp_path):
    from eavsr_amd import harness, ops
    from eavsr_amd.eavsrp_model import EAVSRPModel
    from eavsr_amd.utils.synthetic import synthetic_clip
    ops.lib()
    opt = Namespace(predict=False, n_frame=3, n_flow=5, scale=4, isTrain=True, gpu_ids=[0], lr=1e-4, beta1=0.9, beta2=0.999,
                    weight_decay=0.0, npost=350, checkpoints_dir=str(tmp_path), name="run", optimizer="Adam", load_path="")
    model = EAVSRPModel(opt)
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    items = []
    for k, scene in enumerate(["000", "000", "001"]):
        items.append({"lr_seq": synthetic_clip(1, 3, 64, 64, seed=10 + k), "hr_seq": synthetic_clip(1, 3, 256, 256, seed=20 + k),
                      "fname": [["%s_%05d.png" % (scene, 3 * k + i)] for i in range(3)]})
    rep = harness.evaluate(model, items, per_frame=True, calc_ssim_flag=True, lpips=net)
    # the direct call on the same tensors, and the float64 restatement on the visuals
    sd = R.synthetic_weights(0)
    want, want_ref = [], []
    model.eval()
    for data in items:
        model.set_input(data, 0)
        model.test()
        want += net(model.data_sr_seq, model.data_hr_seq).reshape(-1).tolist()
        vis = {k: v.cpu() for k, v in model.get_current_visuals().items()}
        want_ref += R.lpips(vis["data_sr_seq"][0], vis["data_hr_seq"][0], sd, scale=1.0).tolist()
    assert rep["frame_lpips"] == want and len(want) == 9
    for a, b in zip(want, want_ref):
        print(f"frame lpips {a!r} restatement {b!r}")
        assert abs(a - b) < CAP
    assert [fr["lpips"] for fr in rep["report"]["frames"]] == want
    s0, s1 = sum(want[:6]) / 6, sum(want[6:]) / 3
    assert rep["report"]["scenes"]["000"]["lpips"] == s0 and rep["report"]["scenes"]["001"]["lpips"] == s1
    assert rep["report"]["final"]["lpips"] == (s0 + s1) / 2
    log = open(harness.write_metrics_log(rep["report"], str(tmp_path / "with.txt"))).read()
    assert log.count("  lpips ") == 9 + 2 + 1 and log.endswith("  lpips %.3f\n" % ((s0 + s1) / 2))
    # the same weights from a file named in the options: the default of evaluate
    path = str(tmp_path / "lpips_alex.pth")
    torch.save(sd, path)
    model.opt.lpips_path = path
    again = harness.evaluate(model, items, per_frame=True, calc_ssim_flag=True)
    assert again["frame_lpips"] == want
    del model.opt.lpips_path
    # without lpips: no such keys, and the log of old
    plain = harness.evaluate(model, items, per_frame=True, calc_ssim_flag=True)
    assert "frame_lpips" not in plain and "lpips" not in plain["report"]["final"]
    assert plain["frame_psnr"] == rep["frame_psnr"] and plain["frame_ssim"] == rep["frame_ssim"]
    old = open(harness.write_metrics_log(plain["report"], str(tmp_path / "without.txt"))).read()
    assert "lpips" not in old and old.splitlines() == [ln.split("  lpips ")[0] for ln in log.splitlines()]
    with pytest.raises(ValueError, match="per_frame"):
        harness.evaluate(model, items, lpips=net)
    # an item without HR frames is skipped, as for PSNR and SSIM
    no_hr = harness.evaluate(model, [{"lr_seq": items[0]["lr_seq"], "fname": items[0]["fname"]}], per_frame=True, lpips=net)
    assert no_hr["frame_lpips"] == [] and no_hr["frame_psnr"] == []
