"""Frames of any size on the GPU (`pytest -m gpu`): `ops.ingest_pad` against np.pad and `np.float32(v) / 255` bit for bit,
`EAVSRP.forward_long(pad=...)` / `forward_segments_padded` against the same call on the clip padded by hand (np.pad), cropped,
bit for bit, and `harness.super_resolve(pad=...)` / `harness.evaluate` with `opt.pad_frames` on frames of 66 x 70.

All weights are synthetic; every oracle is numpy (tests/pad_ref.py `pad_oracle`)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import pad_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 8, 8), (2, 2, 64, 64), (1, 3, 4, 4), (33, 35, 64, 64), (66, 70, 68, 72), (64, 64, 64, 64), (7, 9, 7, 10)]
LAYOUTS = ["u8_planes", "u8_interleaved", "f32_planes"]


@pytest.fixture(scope="module")
def ops():
    from eavsr_amd import ops as _ops
    return _ops


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _source(layout, F, C, h, w, seed):
    rng = np.random.default_rng(seed)
    if layout == "u8_interleaved":
        return rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    if layout == "u8_planes":
        return rng.integers(0, 256, (F, C, h, w), dtype=np.uint8)
    x = rng.standard_normal((F, C, h, w)).astype(np.float32)
    flat = x.reshape(-1)
    k = min(3, flat.size)
    flat[:k].view(np.uint32)[:] = (0x7FC01234, 0xFF800000, 0x80000000)[:k]      # a NaN with a payload, -inf, -0: bits are kept
    return x


def _at_offset(x, off, cuda):
    """x on the device as a slice that starts `off` elements past an allocation's (at least 256-byte aligned) start"""
    flat = torch.from_numpy(x).reshape(-1)
    store = torch.zeros(flat.numel() + 8, dtype=flat.dtype, device=cuda)
    store[off:off + flat.numel()] = flat.to(cuda)
    view = store[off:off + flat.numel()].view(x.shape)
    assert view.data_ptr() == store.data_ptr() + off * flat.element_size() and store.data_ptr() % 16 == 0
    return view


# ------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("mode", ["reflect", "edge"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ingest_pad_is_np_pad_over_255_bit_for_bit(ops, cuda, shape, layout, mode):
    """F in {1, 3}, C in {1, 3} (interleaved: 3), sources 0 .. 3 bytes (fp32: samples) past an aligned address"""
    h, w, H, W = shape
    hwc = layout == "u8_interleaved"
    for F in (1, 3):
        for C in ((3,) if hwc else (1, 3)):
            x = _source(layout, F, C, h, w, seed=F * 10 + C)
            want = R.pad_oracle(x, H, W, mode, hwc=hwc)
            for off in (0, 1, 2, 3):
                got = ops.ingest_pad(_at_offset(x, off, cuda), H, W, mode=mode, hwc=hwc)
                assert got.dtype == torch.float32 and tuple(got.shape) == (F, C, H, W) and got.is_contiguous()
                assert np.array_equal(_bits(got).numpy(), want.view(np.int32)), (shape, layout, mode, F, C, off)


@pytest.mark.parametrize("shape", [(64, 64), (7, 9), (66, 72), (5, 1022)], ids=lambda s: "x".join(map(str, s)))
def test_without_padding_it_is_u8_to_f32(ops, cuda, shape):
    """both modes, both byte layouts, every byte alignment; 5 x 1022: rows longer than one pass of a wave, W % 4 != 0"""
    h, w = shape
    for layout in ("u8_planes", "u8_interleaved"):
        x = _source(layout, 2, 3, h, w, seed=7)
        for off in (0, 1, 2, 3):
            src = _at_offset(x, off, cuda)
            want = ops.u8_to_f32(src)
            for mode in ("reflect", "edge"):
                assert torch.equal(_bits(ops.ingest_pad(src, h, w, mode=mode)), _bits(want)), (shape, layout, off, mode)


def test_all_byte_values_and_a_default_layout(ops, cuda):
    """every byte value through the vector and the per-sample path; `hwc=None` reads the layout as `u8_to_f32` does"""
    x = np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16)
    want = R.pad_oracle(x, 20, 24, "reflect")
    assert np.array_equal(_bits(ops.ingest_pad(torch.from_numpy(x).to(cuda), 20, 24)).numpy(), want.view(np.int32))
    want = R.pad_oracle(x, 20, 23, "reflect")
    assert np.array_equal(_bits(ops.ingest_pad(torch.from_numpy(x).to(cuda), 20, 23)).numpy(), want.view(np.int32))
    y = _source("u8_interleaved", 2, 3, 6, 5, seed=1)
    got = ops.ingest_pad(torch.from_numpy(y).to(cuda), 8, 8, mode="edge")
    assert np.array_equal(_bits(got).numpy(), R.pad_oracle(y, 8, 8, "edge", hwc=True).view(np.int32))


def _launches(ops, fn):
    with ops.profile() as prof:
        try:
            out = fn()
        except Exception as e:      # noqa: BLE001 -- handed back to the caller, with what was launched on the way
            out = e
    return out, {k: v["calls"] for k, v in prof.summary().items()}


def test_refused_arguments_and_the_empty_clip_launch_nothing(ops, cuda):
    from eavsr_amd import _native as N
    u8 = torch.zeros(2, 3, 5, 7, dtype=torch.uint8, device=cuda)
    out, launched = _launches(ops, lambda: ops.ingest_pad(u8[:0], 8, 8))
    assert tuple(out.shape) == (0, 3, 8, 8) and out.dtype == torch.float32 and launched == {}
    out, launched = _launches(ops, lambda: ops.ingest_pad(torch.zeros(0, 6, 5, 3, dtype=torch.uint8, device=cuda), 8, 8, hwc=True))
    assert tuple(out.shape) == (0, 3, 8, 8) and launched == {}
    refused = [
        lambda: ops.ingest_pad(u8, 4, 8),                                   # H < h
        lambda: ops.ingest_pad(u8, 8, 6),                                   # W < w
        lambda: ops.ingest_pad(u8, 8, 8, mode="symmetric"),
        lambda: ops.ingest_pad(u8, 8, 8, mode=None),
        lambda: ops.ingest_pad(torch.zeros(2, 5, 7, 4, dtype=torch.uint8, device=cuda), 8, 8, hwc=True),      # interleaved, C != 3
        lambda: ops.ingest_pad(u8.float(), 8, 8, hwc=True),                 # interleaved fp32
        lambda: ops.ingest_pad(u8.to(torch.int16), 8, 8),
        lambda: ops.ingest_pad(u8[0], 8, 8),
        lambda: ops.ingest_pad(u8, 8.0, 8),
    ]
    for i, fn in enumerate(refused):
        out, launched = _launches(ops, fn)
        assert isinstance(out, ValueError) and launched == {}, (i, out, launched)
    # the C entry point refuses the same, and what `ops` cannot hand it: a NULL pointer, a misaligned output, F past a grid dimension
    lib, st = N.load(), torch.cuda.current_stream(cuda).cuda_stream
    dst = torch.full((2 * 3 * 8 * 8 + 4,), -1.0, device=cuda)
    call = lambda src, out, F, C, h, w, Hh, Ww, kind, mode: lib.eavsr_ingest_pad(src, out, F, C, h, w, Hh, Ww, kind, mode, st)
    p, q = u8.data_ptr(), dst.data_ptr()
    assert call(None, q, 2, 3, 5, 7, 8, 8, 0, 0) == -1 and call(p, None, 2, 3, 5, 7, 8, 8, 0, 0) == -1
    for args in ((p, q, 2, 3, 5, 7, 4, 8, 0, 0), (p, q, 2, 3, 5, 7, 8, 6, 0, 0), (p, q, 2, 3, 5, 7, 8, 8, 3, 0), (p, q, 2, 3, 5, 7, 8, 8, 0, 2),
                 (p, q, 2, 4, 5, 7, 8, 8, 1, 0), (p, q + 4, 2, 3, 5, 7, 8, 8, 0, 0), (p, q, 65536, 3, 5, 7, 8, 8, 0, 0),
                 (p, q, -1, 3, 5, 7, 8, 8, 0, 0), (p, q, 2, 3, 0, 7, 8, 8, 0, 0), (p + 1, q, 2, 3, 5, 7, 8, 8, 2, 0)):
        assert call(*args) == -2, args
        assert b"ingest_pad" in lib.eavsr_last_error()
    assert call(p, q, 0, 3, 5, 7, 8, 8, 0, 0) == 0
    torch.cuda.synchronize()
    assert bool((dst == -1.0).all())      # nothing was written by any of them


# ------------------------------------------------------------------------------------------------------------- the model
_NETS = {}


def _net(cuda, tag="x4"):
    if tag not in _NETS:
        from eavsr_amd.eavsrp_model import EAVSRP, EAVSRPx2
        opt = Namespace(predict=False, n_frame=7, n_flow=5, scale=4 if tag == "x4" else 2)
        net = EAVSRP(opt, None) if tag == "x4" else EAVSRPx2(opt, None)
        net.load_state_dict(H.filled(H.model_shapes(tag), "trained_like"), strict=True)
        _NETS[tag] = net.to(cuda).eval()
    return _NETS[tag]


def _clip_u8(n, t, h, w, seed):
    """(n, t, 3, h, w) uint8: `synthetic_clip` at the padded size, its top left corner"""
    from eavsr_amd.utils.synthetic import synthetic_clip
    big = synthetic_clip(n, t, max(64, h + 6), max(64, w + 6), seed=seed)
    return (big[..., :h, :w] * 255).round().to(torch.uint8).contiguous()


def _hand_padded(u8, mode="reflect"):
    """np.pad to `padded_size`, and np.float32(v) / 255: the fp32 clip a user would have built on the host"""
    from eavsr_amd.segments import padded_size
    h, w = u8.shape[-2:]
    Hh, Ww = padded_size(h, w)
    padded = np.pad(u8.numpy(), ((0, 0),) * 3 + ((0, Hh - h), (0, Ww - w)), mode=mode)
    return torch.from_numpy(np.float32(padded) / np.float32(255))


_WANT = {}


def _want(cuda, tag, n, t, h, w, seed, mode="reflect"):
    """(the uint8 clip, `forward_long` of the hand-padded fp32 clip cropped to (s h, s w)): computed once, never written to"""
    key = (tag, n, t, h, w, seed, mode)
    if key not in _WANT:
        u8 = _clip_u8(n, t, h, w, seed)
        net = _net(cuda, tag)
        with torch.no_grad():
            full = net.forward_long(_hand_padded(u8, mode).to(cuda))
        s = net.scale
        _WANT[key] = (u8, full[..., :s * h, :s * w].contiguous())
    return _WANT[key]


@pytest.mark.parametrize("size", [(66, 70), (40, 50)], ids=["66x70", "40x50"])
def test_forward_long_pads_as_the_hand_padded_clip(cuda, size):
    """1 x 3 x 3 x h x w from the three kinds of source, bit for bit; the launches are the hand-padded run's plus one `ingest_pad`"""
    from eavsr_amd import ops
    h, w = size
    u8, want = _want(cuda, "x4", 1, 3, h, w, seed=21)
    net = _net(cuda)
    f32 = torch.from_numpy(np.float32(u8.numpy()) / np.float32(255))
    sources = {"fp32 on the device": f32.to(cuda), "uint8 planes on the device": u8.to(cuda),
               "uint8 interleaved in host memory": u8.permute(0, 1, 3, 4, 2).contiguous().pin_memory()}
    with torch.no_grad():
        for name, src in sources.items():
            with ops.profile() as prof:
                got = net.forward_long(src, pad="reflect")
            assert tuple(got.shape) == (1, 3, 3, 4 * h, 4 * w) and got.is_contiguous(), name
            assert torch.equal(got, want), (name, size)
            calls = {k: v["calls"] for k, v in prof.summary().items()}
            assert calls.get("ingest_pad") == 1 and "u8_to_f32" not in calls, (name, calls)


def test_forward_long_variants_pad_as_the_hand_padded_clip(cuda):
    """66 x 70: frame_chunk=2, cache="host", both (pinned routes: still the whole-batch result), emit=(1, 3), a sink, edge padding"""
    u8, want = _want(cuda, "x4", 1, 3, 66, 70, seed=21)
    net = _net(cuda)
    x = u8.to(cuda)
    with torch.no_grad():
        assert torch.equal(net.forward_long(x, pad="reflect", frame_chunk=2), want)
        assert torch.equal(net.forward_long(x, pad="reflect", cache="host"), want)
        assert torch.equal(net.forward_long(u8.pin_memory(), pad="reflect", frame_chunk=1, cache="host"), want)
        got = net.forward_long(x, pad="reflect", emit=(1, 3))
        assert tuple(got.shape) == (1, 2, 3, 264, 280) and torch.equal(got, want[:, 1:3])
        assert torch.equal(net.forward_long(x, pad="reflect", emit=(1, 3), frame_chunk=2), want[:, 1:3])
        seen = []
        assert net.forward_long(x, pad="reflect", frame_chunk=2, sink=lambda first, sr: seen.append((first, sr))) is None
        assert [f for f, _ in seen] == [0, 2] and all(sr.is_contiguous() for _, sr in seen)
        assert torch.equal(torch.cat([sr for _, sr in seen], 1), want)
        _, want_edge = _want(cuda, "x4", 1, 3, 66, 70, seed=21, mode="edge")
        assert torch.equal(net.forward_long(x, pad="edge"), want_edge)
        assert not torch.equal(want_edge, want)


def test_two_clips_and_the_x2_network(cuda):
    u8, want = _want(cuda, "x4", 2, 3, 66, 70, seed=22)
    with torch.no_grad():
        got = _net(cuda).forward_long(u8.to(cuda), pad="reflect")
        assert tuple(got.shape) == (2, 3, 3, 264, 280) and torch.equal(got, want)
        assert torch.equal(_net(cuda).forward_long(u8.to(cuda), pad="reflect", frame_chunk=2), want)
        u8, want = _want(cuda, "x2", 1, 3, 66, 70, seed=23)
        got = _net(cuda, "x2").forward_long(u8.to(cuda), pad="reflect")
        assert tuple(got.shape) == (1, 3, 3, 132, 140) and torch.equal(got, want)
        u8, want = _want(cuda, "x2", 1, 3, 40, 50, seed=23)
        assert torch.equal(_net(cuda, "x2").forward_long(u8.permute(0, 1, 3, 4, 2).contiguous(), pad="reflect"), want)


def test_forward_segments_pads_every_window(cuda):
    """5 frames of 66 x 70, max_frames=3, overlap=1: the same plan on the hand-padded clip, cropped"""
    from eavsr_amd.segments import plan_segments
    net = _net(cuda)
    u8 = _clip_u8(1, 5, 66, 70, seed=24)
    plan = plan_segments(5, [], 3, 1)
    assert len(plan) > 1
    with torch.no_grad():
        want = net.forward_segments(_hand_padded(u8).to(cuda), plan)[..., :264, :280]
        got = net.forward_segments_padded(u8.to(cuda), plan, "reflect")
        assert tuple(got.shape) == (1, 5, 3, 264, 280) and torch.equal(got, want)
        seen = []
        net.forward_segments_padded(u8.to(cuda), plan, "reflect", sink=lambda first, sr: seen.append((first, sr)))
        assert [f for f, _ in seen] == [ea for _, _, ea, _ in plan] and torch.equal(torch.cat([sr for _, sr in seen], 1), want)


def test_a_size_that_needs_no_padding_runs_as_without_pad(cuda):
    from eavsr_amd import ops
    from eavsr_amd.utils.synthetic import synthetic_clip
    net = _net(cuda)
    x = synthetic_clip(1, 3, 64, 64, seed=25).to(cuda)
    u8 = (x * 255).round().to(torch.uint8)
    with torch.no_grad():
        for src in (x, u8):
            with ops.profile() as prof:
                plain = net.forward_long(src)
            launches = {k: v["calls"] for k, v in prof.summary().items()}
            with ops.profile() as prof:
                padded = net.forward_long(src, pad="reflect")
            assert torch.equal(padded, plain)
            assert {k: v["calls"] for k, v in prof.summary().items()} == launches and "ingest_pad" not in launches


def test_without_pad_other_sizes_are_refused_as_before(cuda):
    net = _net(cuda)
    with torch.no_grad():
        with pytest.raises(ValueError):      # ops.pyramid: h, w divisible by 4
            net.forward_long(_clip_u8(1, 3, 66, 70, seed=21).to(cuda), pad=None)
        with pytest.raises(AssertionError, match="at least 64"):
            net.forward_long(_clip_u8(1, 3, 40, 50, seed=21).to(cuda), pad=None)
        with pytest.raises(AssertionError, match="at least 64"):
            net.forward_segments(_clip_u8(1, 3, 40, 50, seed=21).to(cuda), [(0, 3, 0, 3)])
        with pytest.raises(AssertionError, match="at least 64"):
            net.forward_segments_padded(_clip_u8(1, 3, 40, 50, seed=21).to(cuda), [(0, 3, 0, 3)], None)


# ------------------------------------------------------------------------------------------------------------- the public interface
def _wrapper(**extra):
    from eavsr_amd.eavsrp_model import EAVSRPModel
    model = EAVSRPModel(Namespace(predict=False, n_frame=7, n_flow=5, scale=4, isTrain=False, gpu_ids=[0], **extra))
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    model.eval()
    return model


def _hr_for(u8):
    t = u8.shape[0]
    hr = torch.nn.functional.interpolate(u8.float(), scale_factor=4, mode="bicubic", align_corners=False)
    hr = hr + 4.0 * torch.randn(hr.shape, generator=torch.Generator().manual_seed(3))
    return hr.clamp(0, 255).round().to(torch.uint8).view(t, 3, 4 * u8.shape[2], 4 * u8.shape[3])


def test_super_resolve_of_66x70_png_files(cuda, tmp_path, monkeypatch):
    from eavsr_amd import harness, ops
    from eavsr_amd.lpips import LPIPSAlex
    from tests import lpips_ref
    monkeypatch.delenv("EAVSR_PAD_FRAMES", raising=False)
    lp = LPIPSAlex()
    lp.load_state_dict(lpips_ref.synthetic_weights(0), strict=True)
    lp = lp.to(cuda)
    model = _wrapper()
    u8, want = _want(cuda, "x4", 1, 3, 66, 70, seed=21)
    hr = _hr_for(u8[0])
    names = ["000_%05d.png" % i for i in range(3)]
    paths = [harness.write_png(u8[0, i], str(tmp_path / "lr" / names[i])) for i in range(3)]
    hr_paths = [harness.write_png(hr[i], str(tmp_path / "hr" / names[i])) for i in range(3)]
    want_rgb8 = ops.rgb8(want[0], 255.0)      # (3, 264, 280, 3)
    want_metrics = harness.frame_metrics(want, ops.u8_to_f32(hr.to(cuda)).unsqueeze(0), 255.0, lpips=lp)

    with pytest.raises(ValueError):      # the size is still refused where nothing asks for padding
        harness.super_resolve(model, paths, png_decoder="device")

    def check(res, written=True):
        assert res["frames"] == 3 and res["frame_names"] == names
        assert res["frame_psnr"] == want_metrics["psnr"] and res["frame_ssim"] == want_metrics["ssim"]
        assert res["frame_lpips"] == want_metrics["lpips"]
        if written:
            assert [p.rsplit("/", 1)[1] for p in res["written"]] == names
            decoded = harness.decode_png_frames(res["written"], cuda, channels=3)      # (3, 3, 264, 280)
            assert tuple(decoded.shape) == (3, 3, 264, 280) and torch.equal(decoded.permute(0, 2, 3, 1), want_rgb8)

    for encoder in ("host", "device"):
        res = harness.super_resolve(model, paths, out_dir=str(tmp_path / encoder), hr=hr_paths, lpips=lp, pad="reflect",
                                    png_encoder=encoder, png_decoder="device")
        check(res)
    # scene cuts on the device read the unpadded bytes; the segmented path pads every window
    res = harness.super_resolve(model, paths, out_dir=str(tmp_path / "cuts"), hr=hr_paths, lpips=lp, pad="reflect", cuts="device",
                                png_decoder="device")
    assert [tuple(seg) for seg in res["segments"]] == [(0, 3, 0, 3)]
    check(res)
    hist, sad = harness.scene_changes(u8[0].to(cuda))
    assert int(hist[0].sum()) == 66 * 70
    # the environment alone, the options alone, and the options over the environment
    monkeypatch.setenv("EAVSR_PAD_FRAMES", "reflect")
    check(harness.super_resolve(model, paths, hr=hr_paths, lpips=lp, png_decoder="device"), written=False)
    check(harness.super_resolve(model.netEAVSRP, u8[0], hr=hr, lpips=lp, names=names), written=False)
    monkeypatch.setenv("EAVSR_PAD_FRAMES", "edge")
    model.opt.pad_frames = "reflect"
    check(harness.super_resolve(model, paths, hr=hr_paths, lpips=lp, png_decoder="device"), written=False)
    monkeypatch.delenv("EAVSR_PAD_FRAMES")
    check(harness.super_resolve(model, paths, hr=hr_paths, lpips=lp, png_decoder="device"), written=False)
    del model.opt.pad_frames
    with pytest.raises(ValueError, match="hr frames"):      # hr is expected at (s h, s w), not at the padded size
        harness.super_resolve(model, u8[0], hr=torch.zeros(3, 3, 272, 288, dtype=torch.uint8), pad="reflect")


def test_evaluate_with_pad_frames_on_a_66x70_item(cuda, monkeypatch):
    from eavsr_amd import harness
    monkeypatch.delenv("EAVSR_PAD_FRAMES", raising=False)
    u8, _ = _want(cuda, "x4", 1, 3, 66, 70, seed=21)
    _, want = _want(cuda, "x4", 1, 3, 66, 70, seed=21, mode="edge")
    lr = torch.from_numpy(np.float32(u8.numpy()) / np.float32(255))
    hr = (_hr_for(u8[0]).float() / 255).unsqueeze(0)
    names = ["000_%05d.png" % i for i in range(3)]
    item = {"lr_seq": lr, "hr_seq": hr, "fname": names}
    with pytest.raises(ValueError):
        harness.evaluate(_wrapper(), [item], per_frame=True)
    model = _wrapper(pad_frames="edge")
    rep = harness.evaluate(model, [item], per_frame=True, calc_ssim_flag=True)
    assert tuple(model.data_sr_seq.shape) == (1, 3, 3, 264, 280) and torch.equal(model.data_sr_seq, want)
    fm = harness.frame_metrics(want, hr.to(cuda), 255.0)
    assert rep["frame_psnr"] == fm["psnr"] and rep["frame_ssim"] == fm["ssim"] and rep["frame_names"] == names
    plain = harness.evaluate(model, [item])      # the reference's loop (get_current_visuals) on the cropped frames
    assert len(plain["psnr"]) == 1 and np.isfinite(plain["psnr"][0])
