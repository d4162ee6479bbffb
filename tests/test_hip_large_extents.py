"""Kernels past 2^31 elements / 2^32 bytes (/ 2^32 elements for the cheap streaming ones): the extents where a 32-bit flat index
or byte offset wraps.  Every op here is independent per image, so (tests/large_extents.py, shown to catch a wrap by
tests/test_large_extents_host.py):
  A. the images at the boundaries (first, the ones holding element 2^31 / byte 2^32 / element 2^32, last) are compared with a
     float64 CPU reference of those images alone, under the tolerance the op's existing small-shape test asserts;
  B. the whole-tensor result equals, bit for bit, the same op over x[i:i + chunk] with the route pinned (ops.route_batch), and both
     ran the same kernel names (ops.profile).
Inputs are made on the device chunk by chunk from a seeded generator; no host copy of a whole tensor exists.  No test keeps more
than 64 GiB live; each frees what it made.  Ordered from streaming kernels to convolutions.  The fp32 convolutions are held to
2e-5 * max(1, |ref|max) against float64, also on the F(4x4,3x3) route (whose small-shape test allows 6e-5 against fp32)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import eavsr_oracle as O
from tests import helpers as H
from tests import large_extents as L
from tests import lpips_ref as R
from tests.golden import cases

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
N64, HH, WW = 2740, 96, 128          # 2740 x 64 x 96 x 128 = 2.155e9 elements: past 2^31 (and 2^32 bytes at any element size >= 2)
NPS = 684                            # 684 x 64 x 192 x 256 = 2.152e9: the pixel-shuffled result of a 64 -> 256 convolution
ALL3 = ("elem31", "byte32", "elem32")


@pytest.fixture(scope="module")
def ops(cuda):
    from eavsr_amd import ops as _ops
    _ops.lib()
    if torch.cuda.get_device_properties(0).total_memory < 128 * 2 ** 30:
        pytest.skip("needs a device with at least 128 GiB")
    yield _ops
    print(f"large extents: peak device memory allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def _randn(cuda, shape, seed, chunk=256, dtype=torch.float32):
    return L.fill_chunks(torch.empty(shape, device=cuda, dtype=dtype), lambda t, g: t.normal_(generator=g), seed, chunk)


def _rand(cuda, shape, seed, chunk=256, lo=0.0, hi=1.0):
    return L.fill_chunks(torch.empty(shape, device=cuda), lambda t, g: t.uniform_(lo, hi, generator=g), seed, chunk)


def _bytes(cuda, shape, seed, chunk=1024):
    return L.fill_chunks(torch.empty(shape, device=cuda, dtype=torch.uint8), lambda t, g: t.random_(0, 256, generator=g), seed, chunk)


def _run(ops, label, run, ref, n, chunk, **kw):
    return L.check_extents(label, run, ref, n, chunk, profile=ops.profile, route=ops.route_batch, **kw)


# ------------------------------------------------------------------------------------------------ streaming kernels
def test_add_past_2_32_elements(ops, cuda):
    """torch.equal with the fp32 sum, as test_add"""
    n = 16400                                                    # x 64^3 = 4.299e9 elements, 17.2 GB each; a, b, out: 48 GiB
    a, b = _randn(cuda, (n, 64, 64, 64), 1, 1024), _randn(cuda, (n, 64, 64, 64), 2, 1024)
    rep = _run(ops, "add", lambda lo, hi: ops.add(a[lo:hi], b[lo:hi]), lambda i: a[i].cpu() + b[i].cpu(), n, 2048, must_cross=ALL3)
    assert rep["kernels"] == ["add"]
    del a, b


def test_u8_to_f32_flat_past_2_32_samples(ops, cuda):
    """torch.equal with float(v) / 255 (tests/test_hip_longclip.py's rule)"""
    n = 65535                                                    # x 3 x 128 x 176 = 4.429e9 samples
    x = _bytes(cuda, (n, 3, 128, 176), 3)
    rep = _run(ops, "u8_to_f32 flat", lambda lo, hi: ops.u8_to_f32(x[lo:hi], hwc=False), lambda i: x[i].cpu().float() / 255, n, 8192,
               must_cross=ALL3)
    assert rep["kernels"] == ["u8_to_f32"]
    del x


def test_u8_to_f32_interleaved(ops, cuda):
    n = 65535                                                    # x 112 x 104 x 3 = 2.290e9 samples, 9.2 GB of fp32
    x = _bytes(cuda, (n, 112, 104, 3), 4)
    rep = _run(ops, "u8_to_f32 interleaved", lambda lo, hi: ops.u8_to_f32(x[lo:hi], hwc=True),
         lambda i: x[i].cpu().permute(2, 0, 1).float() / 255, n, 8192)
    assert rep["kernels"] == ['u8_to_f32']
    del x


def test_rgb8(ops, cuda):
    """the quantised frame as bytes: equality with rint(clamp(255 v, 0, 255)), as tests/test_hip_metrics.py"""
    n = 65535
    sr = _rand(cuda, (n, 3, 112, 104), 5, 1024, -0.1, 1.1)
    rep = _run(ops, "rgb8", lambda lo, hi: ops.rgb8(sr[lo:hi]),
         lambda i: torch.clamp(sr[i].cpu() * 255.0, 0, 255).round().to(torch.uint8).permute(1, 2, 0), n, 8192, extent_of=sr,
         must_cross=("elem31", "byte32"))
    assert rep["kernels"] == ['rgb8']
    del sr


def test_normalize_and_avg_pool2(ops, cuda):
    """1e-6 absolute, as test_glue_either_side_of_the_path_matches_aten"""
    n = 21845                                                    # n c = 65535 planes of 176 x 192: 2.215e9 elements
    x = _rand(cuda, (n, 3, 176, 192), 6, 512)
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    mg, sg = mean.to(cuda), std.to(cuda)
    rep = _run(ops, "normalize", lambda lo, hi: ops.normalize(x[lo:hi], mg, sg), lambda i: (x[i].cpu().double() - mean[0].double()) / std[0].double(),
         n, 4096, compare=L.within(1e-6, absolute=True))
    assert rep["kernels"] == ['normalize']
    rep = _run(ops, "avg_pool2", lambda lo, hi: ops.avg_pool2(x[lo:hi]),
         lambda i: F.avg_pool2d(x[i:i + 1].cpu().double(), 2, 2, count_include_pad=False)[0], n, 4096, compare=L.within(1e-6, absolute=True), extent_of=x)
    assert rep["kernels"] == ['avg_pool2']
    del x


def test_resize_bilinear_x4(ops, cuda):
    """2e-6 absolute, as test_glue_either_side_of_the_path_matches_aten; the x4 result crosses"""
    n = 4096                                                     # -> 4096 x 3 x 384 x 512 = 2.416e9 elements
    x = _rand(cuda, (n, 3, 96, 128), 7)
    rep = _run(ops, "resize_bilinear x4", lambda lo, hi: ops.resize_bilinear(x[lo:hi], (384, 512)),
         lambda i: F.interpolate(x[i:i + 1].cpu().double(), size=(384, 512), mode="bilinear", align_corners=False)[0], n, 512, compare=L.within(2e-6, absolute=True))
    assert rep["kernels"] == ['resize_bilinear']
    del x


def test_scale_residual_and_ca_tail(ops, cuda):
    """scale_residual: 1e-5 absolute (test_channel_attention_pieces); ca_tail: 2e-5 max(1, |ref|) (test_ca_tail_one_launch_...)"""
    n = 1023                                                     # n c = 65472 planes of 176 x 192: 2.212e9 elements
    r, x = _randn(cuda, (n, 64, 176, 192), 8, 64), _randn(cuda, (n, 64, 176, 192), 9, 64)
    s = torch.rand(n, 64, generator=torch.Generator().manual_seed(10))
    sg = s.to(cuda)
    rep = _run(ops, "scale_residual", lambda lo, hi: ops.scale_residual(r[lo:hi], sg[lo:hi], x[lo:hi]),
         lambda i: r[i].cpu().double() * s[i].double().view(64, 1, 1) + x[i].cpu().double(), n, 128, compare=L.within(1e-5, absolute=True))
    assert rep["kernels"] == ['scale_residual']
    del r, x
    torch.cuda.empty_cache()
    n, hw = N64, HH * WW
    r, x = _randn(cuda, (n, 64, HH, WW), 11), _randn(cuda, (n, 64, HH, WW), 12)
    part = torch.randn(n, 7, 64, generator=torch.Generator().manual_seed(13)) * (0.05 * hw)
    w1, b1 = cases.randn(72, 4, 64, 1, 1, scale=0.2), cases.randn(73, 4, scale=0.1)
    w2, b2 = cases.randn(74, 64, 4, 1, 1, scale=0.5), cases.randn(75, 64, scale=0.1)
    pg, args = part.to(cuda), [t.to(cuda) for t in (w1, b1, w2, b2)]

    def ref(i):
        mean = (part[i].double().sum(0) / hw).view(1, 64, 1, 1)
        y = torch.sigmoid(F.conv2d(F.relu(F.conv2d(mean, w1.double(), b1.double())), w2.double(), b2.double()))
        return r[i].cpu().double() * y[0] + x[i].cpu().double()
    rep = _run(ops, "ca_tail", lambda lo, hi: ops.ca_tail(r[lo:hi], pg[lo:hi], *args, x[lo:hi]), ref, n, 512, compare=L.within(2e-5))
    assert rep["kernels"] == ["ca_tail"]
    del r, x


def test_to_il8(ops, cuda):
    """torch.equal with the permutation, as test_to_il8_layout"""
    x = _randn(cuda, (N64, 64, HH, WW), 14)
    rep = _run(ops, "to_il8", lambda lo, hi: ops.to_il8(x[lo:hi]), lambda i: x[i].cpu().view(8, 8, HH, WW).permute(0, 2, 3, 1), N64, 512)
    assert rep["kernels"] == ['nchw_to_il8']
    del x


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_layout_converters_h16(ops, cuda, dt):
    """to: torch.equal with the rounded permutation; from (+ residual): 1e-6 absolute -- test_layout_converters_round_trip"""
    x = _randn(cuda, (N64, 64, HH, WW), 15)
    holder = {}

    def to(lo, hi):
        y = ops.to_nhwc_h16(x[lo:hi], dt)
        if hi - lo == N64:
            holder["xh"] = y
        return y
    rep = _run(ops, f"to_nhwc_h16 {dt}", to, lambda i: x[i].cpu().permute(1, 2, 0).to(DT[dt]), N64, 512)
    assert rep["kernels"] == ['nchw_f32_to_nhwc_h16']
    xh = holder.pop("xh")
    del x
    torch.cuda.empty_cache()
    res = _randn(cuda, (N64, 64, HH, WW), 16)
    rep = _run(ops, f"from_nhwc_h16 {dt}", lambda lo, hi: ops.from_nhwc_h16(xh[lo:hi], residual=res[lo:hi]),
         lambda i: xh[i].cpu().double().permute(2, 0, 1) + res[i].cpu().double(), N64, 512, compare=L.within(1e-6, absolute=True))
    assert rep["kernels"] == ['nhwc_h16_to_nchw_f32']
    del xh, res


# ------------------------------------------------------------------------------------------------ ingest and report
def _lpips_rule(per_frame):
    """tests/test_hip_lpips.py's bound: |gpu - ref64| <= max(8 |ref32 - ref64|, 2^-20 |ref64|) on the max-abs of a layer's features
    (check_features), per frame and below 5e-4 for a tap's distance (check_frames); `want` = (ref64, ref32)"""
    def compare(got, want, what):
        r64, r32 = want
        err = (got.double() - r64).abs().max().item()
        bound = max(8 * (r32.double() - r64).abs().max().item(), 2.0 ** -20 * r64.abs().max().item())
        print(f"{what}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound and (not per_frame or err < 5e-4), what
        return err
    compare.rule = "max(8 |ref32 - ref64|, 2^-20 |ref64|)" + (", < 5e-4" if per_frame else "")
    return compare


def test_frame_metrics(ops, cuda):
    """SSE and the 8-bit frame: equality; SSIM: 1e-9 against harness.calc_ssim in float64 (tests/test_hip_metrics.py's bounds)"""
    from eavsr_amd import harness
    n, c, h, w = 58300, 3, 96, 128                               # 2.149e9 samples per tensor
    hr = _rand(cuda, (n, c, h, w), 17, 1024)
    sr = _randn(cuda, (n, c, h, w), 18, 1024)
    for lo in range(0, n, 1024):
        sr[lo:lo + 1024].mul_(4.0 / 255.0).add_(hr[lo:lo + 1024])

    def ref(i):
        q_sr, q_hr = (torch.clamp(t[i].cpu() * 255.0, 0, 255).round() for t in (sr, hr))
        return (((q_sr.long() - q_hr.long()) ** 2).sum(), torch.tensor(harness.calc_ssim(q_sr, q_hr), dtype=torch.float64),
                q_sr.to(torch.uint8).permute(1, 2, 0))
    rep = _run(ops, "frame_metrics", lambda lo, hi: ops.frame_metrics(sr[lo:hi], hr[lo:hi], rgb8=True), ref, n, 8192,
               compare=(L.equal, L.within(1e-9, absolute=True), L.equal), extent_of=sr)
    assert rep["kernels"] == ["frame_metrics"]
    del sr, hr


def test_lpips_conv1_and_tap(ops, cuda):
    """the bounds of tests/test_hip_lpips.py (`_lpips_rule`).  lpips_conv1 returns the SR features then the HR features, so "image i"
    of the helper is the pair (SR_i, HR_i); the images looked at are the pairs one of whose sides holds a boundary of the
    2 f-image feature tensor, and the ones that hold a boundary of the input tensors."""
    f, h, w = 65535, 96, 116                                     # inputs 2.189e9 samples each; features 2 f x 64 x 23 x 28 = 5.40e9
    sd = R.synthetic_weights(0)
    hr = _rand(cuda, (f, 3, h, w), 19, 1024)
    sr = _randn(cuda, (f, 3, h, w), 20, 1024)
    for lo in range(0, f, 1024):
        sr[lo:lo + 1024].mul_(4.0 / 255.0).add_(hr[lo:lo + 1024])
    wt, b = sd["net.slice1.0.weight"].to(cuda), sd["net.slice1.0.bias"].to(cuda)
    shift, scl = sd["scaling_layer.shift"].to(cuda), sd["scaling_layer.scale"].to(cuda)
    lin = sd["lin0.model.1.weight"]
    ling = lin.to(cuda)
    per = 64 * 23 * 28
    images = {k: v % f for k, v in L.boundary_images(2 * f, per, 4).items()}
    images.update({"in:" + k: v for k, v in L.boundary_images(f, 3 * h * w, 4).items()})
    assert all(L.crossed(f, 3 * h * w, 4)[k] for k in ("elem31", "byte32"))
    holder = {}

    def conv1(lo, hi):
        out = ops.lpips_conv1(sr[lo:hi], hr[lo:hi], wt, b, shift, scl)
        if hi - lo == f:
            holder["feat"] = out
        return out.view(2, hi - lo, *out.shape[1:]).transpose(0, 1)

    def ref1(i):
        both = torch.stack([sr[i].cpu(), hr[i].cpu()])
        return tuple(R.layer(R.front_end(both, sd, 255.0, dt), sd, 0) for dt in (torch.float64, torch.float32)),
    rep = _run(ops, "lpips_conv1", conv1, ref1, f, 8192, compare=_lpips_rule(False), extent_of=lambda: holder["feat"], images=images,
               must_cross=ALL3)
    assert rep["kernels"] == ["lpips_conv1"]
    feat = holder.pop("feat")
    assert tuple(feat.shape) == (2 * f, 64, 23, 28)
    del sr, hr
    torch.cuda.empty_cache()

    def tap(lo, hi):
        return ops.lpips_tap(feat if hi - lo == f else torch.cat([feat[lo:hi], feat[f + lo:f + hi]]), ling)

    def ref_tap(i):
        fa, fb = feat[i].cpu()[None], feat[f + i].cpu()[None]
        return (R.tap_distance(fa.double(), fb.double(), lin)[0], R.tap_distance(fa, fb, lin)[0]),
    rep = _run(ops, "lpips_tap", tap, ref_tap, f, 8192, compare=_lpips_rule(True), extent_of=feat, images=images, must_cross=ALL3)
    assert rep["kernels"] == ["lpips_tap"]
    del feat


def test_gather_pairs_from_an_hr_store_above_4_gib(ops, cuda):
    """bit for bit against the numpy restatement of tests/test_hip_dataset.py; frames below, across and above byte 2^32 of the HR
    store, every flip / transpose flag"""
    nf, c, h, w, s, patch = 21900, 3, 64, 64, 4, 48              # HR store 21900 x 3 x 256 x 256 = 4.306e9 bytes
    lr, hr = _bytes(cuda, (nf, c, h, w), 21), _bytes(cuda, (nf, c, s * h, s * w), 22, 512)
    per = c * s * h * s * w
    assert hr.numel() > 2 ** 32
    edge = 2 ** 32 // per                                        # the frame that holds byte 2^32
    assert edge * per < 2 ** 32 < (edge + 1) * per and edge + 2 < nf
    windows = [(0, 1, 2), (edge - 1, edge, edge + 1), (edge, nf - 1, 2 ** 31 // per), (nf - 3, nf - 2, nf - 1)]
    rows = [(win, flags) for win in windows for flags in range(8)]
    frames = np.asarray([win for win, _ in rows], np.int32)
    desc = np.asarray([[(3 * k) % (h - patch + 1), (5 * k + 1) % (w - patch + 1), fl, 0] for k, (_, fl) in enumerate(rows)], np.int32)
    with ops.profile() as prof:
        got_lr, got_hr = ops.gather_pairs(lr, hr, torch.from_numpy(frames).to(cuda), torch.from_numpy(desc).to(cuda), patch, s)
    assert sorted(prof.summary()) == ["gather_pairs_u8"]
    used = sorted(set(frames.reshape(-1).tolist()))
    remap = np.vectorize({v: k for k, v in enumerate(used)}.get)(frames).astype(np.int32)
    lr_small, hr_small = lr[used].cpu().numpy(), hr[used].cpu().numpy()
    print("gather_pairs: HR store", tuple(hr.shape), "bytes", hr.numel(), "frames", used)
    assert torch.equal(got_lr.cpu(), torch.from_numpy(H.restate_pairs(lr_small, remap, desc, patch, patch)))
    assert torch.equal(got_hr.cpu(), torch.from_numpy(H.restate_pairs(hr_small, remap, desc, patch, patch, s)))
    del lr, hr


# ------------------------------------------------------------------------------------------------ count limits
def test_pyramid_folded_launches(ops, cuda):
    """nc = 65535 + 3 planes: the second launch of eavsr_pyramid_f32; 1e-6 absolute on every plane (test_pyramid_matches_interpolate)"""
    x = cases.randn(1, 1, 65538, 4, 8)
    with ops.profile() as prof:
        d2, d4 = ops.pyramid(x.to(cuda))
    assert sorted(prof.summary()) == ["pyramid"]
    r2, r4 = O.feature_pyramid(x)
    assert H.maxabs(d2.cpu(), r2) <= 1e-6 and H.maxabs(d4.cpu(), r4) <= 1e-6


def test_plane_count_limits_raise_and_name_the_limit(ops, cuda):
    """n c = 65536 planes: the library's error, with the limit in it; a small call right after still answers correctly"""
    z = torch.zeros(1, 65536, 2, 4, device=cuda)
    x = cases.randn(2, 2, 3, 8, 12)
    xg = x.to(cuda)
    calls = [
        (lambda t: ops.normalize(t, torch.zeros(t.shape[1], device=cuda), torch.ones(t.shape[1], device=cuda)), lambda: (x - 0) / 1, 1e-6),
        (ops.avg_pool2, lambda: F.avg_pool2d(x, 2, 2), 1e-6),
        (lambda t: ops.resize_bilinear(t, (4, 8)), lambda: F.interpolate(x, size=(4, 8), mode="bilinear", align_corners=False), 2e-6),
        (lambda t: ops.resize_bilinear_ac(t, (4, 8)), lambda: F.interpolate(x, size=(4, 8), mode="bilinear", align_corners=True), 1e-5),
        (lambda t: ops.concat3(t, t[:, :1], t[:, :1]), lambda: torch.cat([x, x[:, :1], x[:, :1]], 1), 0.0),
        (lambda t: ops.scale_residual(t, torch.ones(t.shape[:2], device=cuda), t), lambda: x + x, 1e-5),
    ]
    for call, want, tol in calls:
        with pytest.raises(RuntimeError, match="65535"):
            call(z)
        assert H.maxabs(call(xg).cpu(), want()) <= tol


# ------------------------------------------------------------------------------------------------ 16-bit backbone layer kernels
def _h16_compare(dt):
    """test_conv3x3_c64_h16_vs_fp32_on_rounded_inputs' bound: one rounding to 16 bits (+ 1e-5 of fp32 summation-order noise)"""
    return L.within(EPS[dt] * 1.01, extra=1e-5)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_conv3x3_c64_h16(ops, cuda, dt):
    xh = _randn(cuda, (N64, HH, WW, 64), 30, dtype=DT[dt])
    wt, b = cases.randn(2, 64, 64, 3, 3, scale=1.0 / 24.0), cases.randn(3, 64, scale=0.1)
    wg, bg, wr = wt.to(cuda), b.to(cuda), wt.to(DT[dt]).double()
    ref = lambda i: F.relu(F.conv2d(xh[i:i + 1].cpu().double().permute(0, 3, 1, 2), wr, b.double(), 1, 1))[0].permute(1, 2, 0)
    rep = _run(ops, f"conv3x3_c64_h16 {dt}", lambda lo, hi: ops.conv3x3_c64_h16(xh[lo:hi], wg, bg, relu=True), ref, N64, 512,
               compare=_h16_compare(dt))
    assert rep["kernels"] == ["conv3x3_64to64_h16"]
    del xh


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_conv3x3_c64_h16_act_pixel_shuffle(ops, cuda, dt):
    xh = _randn(cuda, (NPS, HH, WW, 64), 31, dtype=DT[dt])
    w4, b4 = cases.randn(14, 256, 64, 3, 3, scale=1.0 / 24.0), cases.randn(15, 256, scale=0.1)
    wg, bg, wr = w4.to(cuda), b4.to(cuda), w4.to(DT[dt]).double()
    ref = lambda i: F.leaky_relu(F.pixel_shuffle(F.conv2d(xh[i:i + 1].cpu().double().permute(0, 3, 1, 2), wr, b4.double(), 1, 1), 2),
                                 0.1)[0].permute(1, 2, 0)
    rep = _run(ops, f"conv3x3_c64_h16_act ps2 {dt}",
               lambda lo, hi: ops.conv3x3_c64_h16_act(xh[lo:hi], wg, bg, act="lrelu", slope=0.1, pixel_shuffle2=True), ref, NPS, 128,
               compare=_h16_compare(dt))
    assert rep["kernels"] == ["conv3x3_64to256_h16_ps2"]
    del xh


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_conv3x3_c64to3_h16(ops, cuda, dt):
    """2e-5 max(1, |ref|) against float64 on the rounded operands (test_conv3x3_c64to3_h16_vs_fp64_on_rounded_inputs)"""
    xh = _randn(cuda, (N64, HH, WW, 64), 32, dtype=DT[dt])
    res = _randn(cuda, (N64, 3, HH, WW), 33)
    wt, b = cases.randn(22, 3, 64, 3, 3, scale=1.0 / 24.0), cases.randn(23, 3, scale=0.1)
    wg, bg, wr = wt.to(cuda), b.to(cuda), wt.to(DT[dt]).double()
    ref = lambda i: F.conv2d(xh[i:i + 1].cpu().double().permute(0, 3, 1, 2), wr, b.double(), 1, 1)[0] + res[i].cpu().double()
    rep = _run(ops, f"conv3x3_c64to3_h16 {dt}", lambda lo, hi: ops.conv3x3_c64to3_h16(xh[lo:hi], wg, bg, residual=res[lo:hi]), ref, N64, 512,
               compare=L.within(2e-5), extent_of=xh)
    assert rep["kernels"] == ["conv3x3_64to3_h16"]
    del xh, res


# ------------------------------------------------------------------------------------------------ fp32 convolutions
def _conv_ref(x, i, wt, b, act=None):
    y = F.conv2d(x[i:i + 1].cpu().double(), wt.double(), b.double(), 1, 1)
    return F.leaky_relu(y, 0.1) if act == "lrelu" else y


def test_conv_3_to_64(ops, cuda):
    x = _randn(cuda, (N64, 3, HH, WW), 40)
    wt, b = cases.randn(41, 64, 3, 3, 3, scale=1.0 / 27 ** 0.5), cases.randn(42, 64, scale=0.1)
    wg, bg = wt.to(cuda), b.to(cuda)
    rep = _run(ops, "conv 3->64", lambda lo, hi: ops.conv2d(x[lo:hi], wg, bg), lambda i: _conv_ref(x, i, wt, b)[0], N64, 512, compare=L.within(2e-5))
    assert rep["kernels"] == ['conv3x3_3to64']
    del x


def test_conv_64_to_3_small_cout_with_residual(ops, cuda):
    x, res = _randn(cuda, (N64, 64, HH, WW), 43), _randn(cuda, (N64, 3, HH, WW), 44)
    wt, b = cases.randn(45, 3, 64, 3, 3, scale=1.0 / 24.0), cases.randn(46, 3, scale=0.1)
    wg, bg = wt.to(cuda), b.to(cuda)
    rep = _run(ops, "conv 64->3 smallco", lambda lo, hi: ops.conv2d(x[lo:hi], wg, bg, residual=res[lo:hi]),
         lambda i: _conv_ref(x, i, wt, b)[0] + res[i].cpu().double(), N64, 512, compare=L.within(2e-5), extent_of=x)
    assert rep["kernels"] == ['conv3x3_64to3']
    # the profile name is shared by the small-cout kernels: conv2d sends cout = 3 to them unconditionally, and this is the gate of
    # the co-resident one (eavsr_conv3x3_smallco_lite_f32), which holds at this size
    assert ops.SMALLCO_LITE and HH * WW * 64 * 4 < 2 ** 32 and N64 * (HH // 8) * (WW // 64) >= ops.SMALLCO_LITE_MIN_TILES
    del x, res


def test_conv_64_to_256_pixel_shuffle(ops, cuda):
    x = _randn(cuda, (NPS, 64, HH, WW), 47)
    wt, b = cases.randn(48, 256, 64, 3, 3, scale=1.0 / 24.0), cases.randn(49, 256, scale=0.1)
    wg, bg = wt.to(cuda), b.to(cuda)
    rep = _run(ops, "conv 64->256 ps2", lambda lo, hi: ops.conv2d(x[lo:hi], wg, bg, act="lrelu", slope=0.1, pixel_shuffle2=True),
               lambda i: F.pixel_shuffle(_conv_ref(x, i, wt, b, "lrelu"), 2)[0], NPS, 128, compare=L.within(2e-5))
    assert rep["kernels"] == ["conv3x3_64to256_wino4"]
    del x


def test_conv_64_to_64_winograd4_residual_res_scale(ops, cuda):
    x, res = _randn(cuda, (N64, 64, HH, WW), 50), _randn(cuda, (N64, 64, HH, WW), 51)
    s = torch.rand(N64, 64, generator=torch.Generator().manual_seed(52))
    sg = s.to(cuda)
    wt, b = cases.randn(53, 64, 64, 3, 3, scale=1.0 / 24.0), cases.randn(54, 64, scale=0.1)
    wg, bg = wt.to(cuda), b.to(cuda)
    rep = _run(ops, "conv 64->64 wino4 res_scale", lambda lo, hi: ops.conv2d(x[lo:hi], wg, bg, residual=res[lo:hi], res_scale=sg[lo:hi]),
               lambda i: res[i].cpu().double() + s[i].double().view(64, 1, 1) * _conv_ref(x, i, wt, b)[0], N64, 512, compare=L.within(2e-5))
    assert rep["kernels"] == ["conv3x3_64to64_wino4"]
    del x, res


def test_conv_64_to_64_direct_mode(ops, cuda):
    x = _randn(cuda, (N64, 64, HH, WW), 55)
    wt, b = cases.randn(56, 64, 64, 3, 3, scale=1.0 / 24.0), cases.randn(57, 64, scale=0.1)
    wg, bg = wt.to(cuda), b.to(cuda)
    with ops.modes(conv="direct"):
        rep = _run(ops, "conv 64->64 direct", lambda lo, hi: ops.conv2d(x[lo:hi], wg, bg), lambda i: _conv_ref(x, i, wt, b)[0], N64, 512,
                   compare=L.within(2e-5))
    assert rep["kernels"] == ["conv3x3_64to64"]
    del x
