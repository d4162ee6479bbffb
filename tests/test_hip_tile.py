"""Frames of any resolution on the GPU (`pytest -m gpu`): `ops.ingest_window` and `ops.tile_blend` against their numpy
restatements (tests/tile_ref.py) bit for bit, `EAVSRP.forward_tiled` against the tile_ref blend of `forward_long` on the
hand-cropped clips bit for bit, and `harness.super_resolve(tile=...)` / `harness.evaluate` with `opt.tile` on frames of 96 x 112.

All weights are synthetic; every oracle is numpy."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import tile_ref as R

pytestmark = pytest.mark.gpu

LAYOUTS = ["u8_planes", "u8_interleaved", "f32_planes"]


@pytest.fixture(scope="module")
def ops():
    from eavsr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_on_the_device():
    """the networks and reference tensors this module caches are dropped when it ends, and the allocator's blocks with them: the
    files that run after it find the device as they would without it"""
    yield
    _NETS.clear()
    _WANT.clear()
    torch.cuda.empty_cache()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _source(layout, F, C, h, w, seed):
    rng = np.random.default_rng(seed)
    if layout == "u8_interleaved":
        return rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    if layout == "u8_planes":
        return rng.integers(0, 256, (F, C, h, w), dtype=np.uint8)
    x = rng.standard_normal((F, C, h, w)).astype(np.float32)
    x.reshape(-1)[:3].view(np.uint32)[:] = (0x7FC01234, 0xFF800000, 0x80000000)      # a NaN with a payload, -inf, -0: bits are kept
    return x


def _at_offset(x, off, cuda):
    """x on the device as a slice that starts `off` elements past an allocation's (at least 256-byte aligned) start"""
    flat = torch.from_numpy(x).reshape(-1)
    store = torch.zeros(flat.numel() + 8, dtype=flat.dtype, device=cuda)
    store[off:off + flat.numel()] = flat.to(cuda)
    view = store[off:off + flat.numel()].view(x.shape)
    assert view.data_ptr() == store.data_ptr() + off * flat.element_size() and store.data_ptr() % 16 == 0
    return view


def _launches(ops, fn):
    with ops.profile() as prof:
        try:
            out = fn()
        except Exception as e:      # noqa: BLE001 -- handed back to the caller, with what was launched on the way
            out = e
    return out, {k: v["calls"] for k, v in prof.summary().items()}


# ------------------------------------------------------------------------------------------------------------- ingest_window
@pytest.mark.parametrize("mode", ["reflect", "edge"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ingest_window_is_slicing_then_np_pad_over_255_bit_for_bit(ops, cuda, layout, mode):
    """frames of 70 x 83 (a pitch that is no multiple of 4), F and C in {1, 3}, windows at x0 in {0, 1, 2, 3, 19} and y0 in {0, 5},
    sources 0 .. 3 bytes (fp32: samples) past an aligned address; windows of 64 columns into outputs of 64 and 68 (one reflected
    quad), and of 62 columns into 64"""
    hwc = layout == "u8_interleaved"
    for F, C in ((1, 3), (3, 3)) if hwc else ((1, 1), (3, 3), (1, 3), (3, 1)):
        x = _source(layout, F, C, 70, 83, seed=F * 10 + C)
        srcs = [_at_offset(x, off, cuda) for off in (0, 1, 2, 3)]
        for y0 in (0, 5):
            for x0 in (0, 1, 2, 3, 19):
                for ww, W in ((64, 64), (64, 68), (62, 64)):
                    want = R.window_oracle(x, y0, x0, 64, ww, 64, W, mode, hwc=hwc).view(np.int32)
                    for off, src in enumerate(srcs):
                        got = ops.ingest_window(src, y0, x0, 64, ww, 64, W, mode=mode, hwc=hwc)
                        assert got.dtype == torch.float32 and tuple(got.shape) == (F, C, 64, W) and got.is_contiguous()
                        assert np.array_equal(_bits(got).numpy(), want), (layout, mode, F, C, y0, x0, ww, W, off)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_window_that_spans_a_short_axis_is_padded_and_slicing_then_ingest_pad_gives_the_same_bits(ops, cuda, layout):
    """frames of 50 x 83: the window spans the 50 rows and is padded to 64 in both modes; for every window, ingest_window is
    ingest_pad of the slice's contiguous copy; the whole frame as the window is ingest_pad itself; an odd output width (W % 4 != 0)"""
    hwc = layout == "u8_interleaved"
    x = _source(layout, 2, 3, 50, 83, seed=5)
    src = torch.from_numpy(x).to(cuda)
    for mode in ("reflect", "edge"):
        for x0, ww, W in ((0, 64, 64), (19, 64, 64), (3, 70, 72), (0, 83, 84), (7, 61, 63)):
            want = R.window_oracle(x, 0, x0, 50, ww, 64, W, mode, hwc=hwc)
            got = ops.ingest_window(src, 0, x0, 50, ww, 64, W, mode=mode, hwc=hwc)
            assert np.array_equal(_bits(got).numpy(), want.view(np.int32)), (layout, mode, x0, ww, W)
            part = (src[:, :, x0:x0 + ww] if hwc else src[..., x0:x0 + ww]).contiguous()
            assert torch.equal(_bits(ops.ingest_pad(part, 64, W, mode=mode, hwc=hwc)), _bits(got))
    assert torch.equal(_bits(ops.ingest_window(src, 0, 0, 50, 83, mode="edge", hwc=hwc)), _bits(ops.ingest_pad(src, 50, 83, mode="edge", hwc=hwc)))
    got = ops.ingest_window(src, 5, 2, 40, 64)      # H, W default to the window; the layout is read as `u8_to_f32` reads it
    assert np.array_equal(_bits(got).numpy(), R.window_oracle(x, 5, 2, 40, 64, 40, 64, "reflect", hwc=hwc).view(np.int32))


# (h, w, H, W) of F = 2, C = 3 frames: the smallest shapes that reach every path of the one kernel family behind both ops
_ONE_KERNEL_SHAPES = [
    (5, 7, 8, 12),        # vector stores; the reflected quads straddle the last column
    (5, 7, 7, 9),         # W % 4 != 0: one sample per lane
    (3, 5, 16, 20),       # padding several times the size: the reflect period wraps
    (4, 264, 4, 264),     # nothing to pad; more than one pass of 64 lanes x 4 samples
    (1, 1, 4, 4),         # s == 1
]


@pytest.mark.parametrize("mode", ["reflect", "edge"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ingest_pad_is_ingest_window_of_the_whole_frame_bit_for_bit(ops, cuda, layout, mode):
    """`ops.ingest_pad(x, H, W)` and `ops.ingest_window(x, 0, 0, h, w, H, W)` give the same bits, and both are tests/pad_ref.py's
    np.pad statement (so they cannot be wrong together): at an aligned base and at one sliced 1 byte (fp32: 1 sample, which takes
    the 16-byte alignment away; an fp32 source is 4-byte aligned by contract) past it"""
    from tests import pad_ref
    hwc = layout == "u8_interleaved"
    for h, w, Hh, Ww in _ONE_KERNEL_SHAPES:
        x = _source(layout, 2, 3, h, w, seed=h * 1000 + w)
        want = pad_ref.pad_oracle(x, Hh, Ww, mode, hwc=hwc).view(np.int32)
        for off in (0, 1):
            src = _at_offset(x, off, cuda)
            assert src.data_ptr() % 2 == off or src.dtype == torch.float32
            padded = ops.ingest_pad(src, Hh, Ww, mode=mode, hwc=hwc)
            windowed = ops.ingest_window(src, 0, 0, h, w, Hh, Ww, mode=mode, hwc=hwc)
            assert tuple(padded.shape) == tuple(windowed.shape) == (2, 3, Hh, Ww)
            assert torch.equal(_bits(padded), _bits(windowed)), (layout, mode, h, w, Hh, Ww, off)
            assert np.array_equal(_bits(padded).numpy(), want), (layout, mode, h, w, Hh, Ww, off)


def test_ingest_window_refusals_launch_nothing(ops, cuda):
    from eavsr_amd import _native as N
    u8 = torch.zeros(2, 3, 20, 30, dtype=torch.uint8, device=cuda)
    out, launched = _launches(ops, lambda: ops.ingest_window(u8[:0], 0, 0, 8, 8))
    assert tuple(out.shape) == (0, 3, 8, 8) and out.dtype == torch.float32 and launched == {}
    refused = [
        lambda: ops.ingest_window(u8, 13, 0, 8, 8),               # y0 + wh > h
        lambda: ops.ingest_window(u8, 0, 23, 8, 8),               # x0 + ww > w
        lambda: ops.ingest_window(u8, -1, 0, 8, 8),
        lambda: ops.ingest_window(u8, 0, 0, 0, 8),
        lambda: ops.ingest_window(u8, 0, 0, 8, 8, 4, 8),          # H < wh
        lambda: ops.ingest_window(u8, 0, 0, 8, 8, 8, 6),          # W < ww
        lambda: ops.ingest_window(u8, 0, 0, 8, 8, mode="symmetric"),
        lambda: ops.ingest_window(u8.float(), 0, 0, 8, 8, hwc=True),
        lambda: ops.ingest_window(u8.to(torch.int16), 0, 0, 8, 8),
        lambda: ops.ingest_window(u8[0], 0, 0, 8, 8),
        lambda: ops.ingest_window(u8, 0.0, 0, 8, 8),
    ]
    for i, fn in enumerate(refused):
        out, launched = _launches(ops, fn)
        assert isinstance(out, ValueError) and launched == {}, (i, out, launched)
    lib, st = N.load(), torch.cuda.current_stream(cuda).cuda_stream
    dst = torch.full((2 * 3 * 8 * 8 + 4,), -1.0, device=cuda)
    p, q = u8.data_ptr(), dst.data_ptr()
    call = lambda *a: lib.eavsr_ingest_window(*a, st)
    assert call(None, q, 2, 3, 20, 30, 0, 0, 8, 8, 8, 8, 0, 0) == -1 and call(p, None, 2, 3, 20, 30, 0, 0, 8, 8, 8, 8, 0, 0) == -1
    for args in ((p, q, 2, 3, 20, 30, 13, 0, 8, 8, 8, 8, 0, 0), (p, q, 2, 3, 20, 30, 0, 23, 8, 8, 8, 8, 0, 0), (p, q, 2, 3, 20, 30, -1, 0, 8, 8, 8, 8, 0, 0),
                 (p, q, 2, 3, 20, 30, 0, 0, 8, 8, 4, 8, 0, 0), (p, q, 2, 3, 20, 30, 0, 0, 8, 8, 8, 8, 3, 0), (p, q, 2, 3, 20, 30, 0, 0, 8, 8, 8, 8, 0, 2),
                 (p, q, 2, 4, 20, 30, 0, 0, 8, 8, 8, 8, 1, 0), (p, q + 4, 2, 3, 20, 30, 0, 0, 8, 8, 8, 8, 0, 0), (p, q, 65536, 3, 20, 30, 0, 0, 8, 8, 8, 8, 0, 0),
                 (p + 1, q, 2, 3, 20, 30, 0, 0, 8, 8, 8, 8, 2, 0), (p, q, 2, 3, 20, 30, 2 ** 31 - 1, 0, 8, 8, 8, 8, 0, 0)):
        assert call(*args) == -2, args
        assert b"ingest_window" in lib.eavsr_last_error()
    assert call(p, q, 0, 3, 20, 30, 0, 0, 8, 8, 8, 8, 0, 0) == 0
    torch.cuda.synchronize()
    assert bool((dst == -1.0).all())


# ------------------------------------------------------------------------------------------------------------- tile_blend
def _strided_tile(rng, n, F, C, th, tw, cuda):
    """(numpy (n, F, C, th, tw), the device view): the top left of frame-major (F, n, C, th + 4, tw + 4) frames, transposed -- the
    cropped, transposed view `forward_long` holds"""
    full = rng.standard_normal((F, n, C, th + 4, tw + 4)).astype(np.float32)
    dev = torch.from_numpy(full).to(cuda)
    view = dev.transpose(0, 1)[..., :th, :tw]
    assert not view.is_contiguous() and view.stride(-1) == 1
    return np.ascontiguousarray(full.transpose(1, 0, 2, 3, 4)[..., :th, :tw]), view


@pytest.mark.parametrize("X0", [0, 2, 4, 50])
def test_tile_blend_is_the_numpy_statement_bit_for_bit(ops, cuda, X0):
    """four overlapped tiles (widths 64 and 68, strided sources) accumulated in order into 2 x 3 x 3 x 136 x 200; a second run gives
    the same bits; contiguous sources and 1 x 1 planes too"""
    rng = np.random.default_rng(X0)
    n, F, C = 2, 3, 3
    acc0 = rng.standard_normal((n, F, C, 136, 200)).astype(np.float32)
    tiles = [(0, X0, 64, 64), (0, X0 + 40, 64, 68), (60, X0, 68, 64), (72, X0 + 38, 64, 68)]
    want, runs = acc0.copy(), []
    parts = []
    for Y0, x0, th, tw in tiles:
        sr_np, sr_dev = _strided_tile(rng, n, F, C, th, tw, cuda)
        wy, wx = rng.random(th, dtype=np.float32), rng.random(tw, dtype=np.float32)
        R.blend_oracle(want, sr_np, Y0, x0, wy, wx)
        parts.append((Y0, x0, sr_dev, torch.from_numpy(wy).to(cuda), torch.from_numpy(wx).to(cuda)))
    for _ in range(2):
        acc = torch.from_numpy(acc0).to(cuda)
        for Y0, x0, sr_dev, wy, wx in parts:
            assert ops.tile_blend(acc, sr_dev, Y0, x0, wy, wx) is acc
        runs.append(_bits(acc))
    assert np.array_equal(runs[0].numpy(), want.view(np.int32)) and torch.equal(runs[0], runs[1])
    acc = torch.from_numpy(acc0).to(cuda)      # the same tiles as contiguous tensors
    for Y0, x0, sr_dev, wy, wx in parts:
        ops.tile_blend(acc, sr_dev.contiguous(), Y0, x0, wy, wx)
    assert torch.equal(_bits(acc), runs[0])
    one = torch.from_numpy(acc0[:1, :1, :1].copy()).to(cuda)
    Y0, x0, sr_dev, wy, wx = parts[1]
    ops.tile_blend(one, sr_dev[:1, :1, :1], Y0, x0, wy, wx)
    ref = R.blend_oracle(acc0[:1, :1, :1].copy(), sr_dev[:1, :1, :1].cpu().numpy(), Y0, x0, wy.cpu().numpy(), wx.cpu().numpy())
    assert np.array_equal(_bits(one).numpy(), ref.view(np.int32))


@pytest.mark.parametrize("X0", [0, 1, 2, 4])
def test_tile_blend_rows_longer_than_a_pass_and_every_alignment(ops, cuda, X0):
    """width 256 + 4 (a second pass of the lane loop) and 256 + 6 (and a tail of 2), into 1 x 2 x 3 x 70 x 301 (an odd pitch: the
    rows' alignment changes from row to row); weights at 4-, 8- and 16-byte aligned addresses"""
    rng = np.random.default_rng(10 + X0)
    for tw in (260, 262):
        acc0 = rng.standard_normal((1, 2, 3, 70, 301)).astype(np.float32)
        sr_np, sr_dev = _strided_tile(rng, 1, 2, 3, 66, tw, cuda)
        wy = rng.random(66, dtype=np.float32)
        wx = rng.random(tw, dtype=np.float32)
        want = R.blend_oracle(acc0.copy(), sr_np, 3, X0, wy, wx)
        for off in (0, 1, 2):
            acc = torch.from_numpy(acc0).to(cuda)
            ops.tile_blend(acc, sr_dev, 3, X0, _at_offset(wy, off, cuda), _at_offset(wx, off, cuda))
            assert np.array_equal(_bits(acc).numpy(), want.view(np.int32)), (X0, tw, off)


def test_tile_blend_refusals_launch_nothing(ops, cuda):
    acc = torch.zeros(1, 2, 3, 16, 24, device=cuda)
    sr = torch.ones(1, 2, 3, 8, 12, device=cuda)
    wy, wx = torch.ones(8, device=cuda), torch.ones(12, device=cuda)
    refused = [
        lambda: ops.tile_blend(acc, sr, 9, 0, wy, wx),                      # leaves the frame
        lambda: ops.tile_blend(acc, sr, 0, 13, wy, wx),
        lambda: ops.tile_blend(acc, sr, -1, 0, wy, wx),
        lambda: ops.tile_blend(acc, sr, 0, 0, wx, wy),                      # weights of the wrong length
        lambda: ops.tile_blend(acc, sr[:, :1], 0, 0, wy, wx),               # other planes
        lambda: ops.tile_blend(acc[..., :20], sr, 0, 0, wy, wx),            # acc is not contiguous
        lambda: ops.tile_blend(acc, sr.transpose(3, 4).contiguous().transpose(3, 4), 0, 0, wy, wx),      # no unit stride along x
        lambda: ops.tile_blend(acc, sr.double(), 0, 0, wy, wx),
        lambda: ops.tile_blend(acc, sr, 0.0, 0, wy, wx),
        lambda: ops.tile_blend(acc[0], sr[0], 0, 0, wy, wx),
    ]
    for i, fn in enumerate(refused):
        out, launched = _launches(ops, fn)
        assert isinstance(out, ValueError) and launched == {}, (i, out, launched)
    out, launched = _launches(ops, lambda: ops.tile_blend(acc[:, :0], sr[:, :0], 0, 0, wy, wx))
    assert launched == {} and bool((acc == 0).all())


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
    from eavsr_amd.utils.synthetic import synthetic_clip
    big = synthetic_clip(n, t, h + (-h) % 4 + 4, w + (-w) % 4 + 4, seed=seed)
    return (big[..., :h, :w] * 255).round().to(torch.uint8).contiguous()


_WANT = {}


def _want(cuda, tag, n, t, h, w, seed, tile, overlap, pad=None, plan=None):
    """(the uint8 clip, the tile_ref blend of `forward_long` / `forward_segments_padded` on each hand-cropped clip, on the device):
    computed once, never written to"""
    key = (tag, n, t, h, w, seed, tile, overlap, pad, None if plan is None else tuple(plan))
    if key not in _WANT:
        u8 = _clip_u8(n, t, h, w, seed)
        net = _net(cuda, tag)
        tiles = R.plan_tiles(h, w, tile, overlap)
        per_tile = []
        with torch.no_grad():
            for y0, y1, x0, x1 in tiles:
                crop = u8[..., y0:y1, x0:x1].contiguous().to(cuda)
                sr = net.forward_long(crop, pad=pad) if plan is None else net.forward_segments_padded(crop, plan, pad)
                per_tile.append(sr.cpu().numpy())
        _WANT[key] = (u8, torch.from_numpy(R.blend_tiles(per_tile, tiles, h, w, net.scale, tile, overlap)).to(cuda))
    return _WANT[key]


def test_forward_tiled_is_the_blend_of_forward_long_on_hand_cropped_windows(cuda):
    """1 x 3 x 3 x 96 x 112, tile 64, overlap 16 -- a 2 x 2 plan -- from uint8 planes, uint8 interleaved in host memory and fp32, bit for
    bit; the launches: one `ingest_window` and one `tile_blend` per tile, no `u8_to_f32`"""
    from eavsr_amd import ops
    u8, want = _want(cuda, "x4", 1, 3, 96, 112, 31, 64, 16)
    net = _net(cuda)
    f32 = torch.from_numpy(np.float32(u8.numpy()) / np.float32(255))
    sources = {"uint8 planes on the device": u8.to(cuda), "fp32 on the device": f32.to(cuda),
               "uint8 interleaved in host memory": u8.permute(0, 1, 3, 4, 2).contiguous().pin_memory(),
               "uint8 interleaved on the device": u8.permute(0, 1, 3, 4, 2).contiguous().to(cuda), "uint8 planes in host memory": u8}
    with torch.no_grad():
        for name, src in sources.items():
            with ops.profile() as prof:
                got = net.forward_tiled(src, 64, overlap=16)
            assert tuple(got.shape) == (1, 3, 3, 384, 448) and got.is_contiguous(), name
            assert torch.equal(_bits(got), _bits(want)), name
            calls = {k: v["calls"] for k, v in prof.summary().items()}
            assert calls.get("ingest_window") == 4 and calls.get("tile_blend") == 4 and "u8_to_f32" not in calls, (name, calls)
        whole = net.forward_long(u8.to(cuda))
    assert not torch.equal(got, whole)      # it is NOT the whole-frame result: a tile's network sees the tile alone


def test_one_tile_is_forward_long_and_blends_nothing(cuda):
    from eavsr_amd import ops
    from eavsr_amd.segments import plan_segments
    net = _net(cuda)
    u8 = _clip_u8(1, 3, 96, 112, 31).to(cuda)
    with torch.no_grad():
        with ops.profile() as prof:
            plain = net.forward_long(u8)
        launches = {k: v["calls"] for k, v in prof.summary().items()}
        with ops.profile() as prof:
            tiled = net.forward_tiled(u8, 128, overlap=32)
        assert torch.equal(tiled, plain)
        got = {k: v["calls"] for k, v in prof.summary().items()}
        assert got == launches and "tile_blend" not in got and "ingest_window" not in got
        plan = plan_segments(3, [], 2, 1)
        assert torch.equal(net.forward_tiled(u8, (96, 112), segments=plan), net.forward_segments(u8, plan))


def test_forward_tiled_variants(cuda):
    """frame_chunk=2, cache="host", both, and a sink: the same tensor"""
    u8, want = _want(cuda, "x4", 1, 3, 96, 112, 31, 64, 16)
    net = _net(cuda)
    x = u8.to(cuda)
    with torch.no_grad():
        assert torch.equal(net.forward_tiled(x, 64, overlap=16, frame_chunk=2), want)
        assert torch.equal(net.forward_tiled(x, 64, overlap=16, cache="host"), want)
        assert torch.equal(net.forward_tiled(u8.pin_memory(), (64, 64), overlap=16, frame_chunk=1, cache="host"), want)
        seen = []
        assert net.forward_tiled(x, 64, overlap=16, frame_chunk=2, sink=lambda first, sr: seen.append((first, sr))) is None
        assert [f for f, _ in seen] == [0, 2] and all(sr.is_contiguous() for _, sr in seen)
        assert torch.equal(torch.cat([sr for _, sr in seen], 1), want)


def test_two_clips(cuda):
    u8, want = _want(cuda, "x4", 2, 3, 96, 112, 32, 64, 16)
    with torch.no_grad():
        got = _net(cuda).forward_tiled(u8.to(cuda), 64, overlap=16)
        assert tuple(got.shape) == (2, 3, 3, 384, 448) and torch.equal(got, want)
        assert torch.equal(_net(cuda).forward_tiled(u8.to(cuda), 64, overlap=16, frame_chunk=2), want)      # blended clip by clip


def test_a_two_segment_plan(cuda):
    """4 frames, windows of 3 that share 2: per tile the segmented run on the hand-cropped clip; one accumulator serves both
    segments, and a sink that keeps its chunks is not overwritten"""
    from eavsr_amd.segments import plan_segments
    plan = plan_segments(4, [], 3, 2)
    assert len(plan) == 2
    u8, want = _want(cuda, "x4", 1, 4, 96, 112, 33, 64, 16, plan=plan)
    net = _net(cuda)
    with torch.no_grad():
        got = net.forward_tiled(u8.to(cuda), 64, overlap=16, segments=plan)
        assert tuple(got.shape) == (1, 4, 3, 384, 448) and torch.equal(got, want)
        seen = []
        net.forward_tiled(u8, 64, overlap=16, segments=plan, sink=lambda first, sr: seen.append((first, sr)))
        assert [f for f, _ in seen] == [ea for _, _, ea, _ in plan] and torch.equal(torch.cat([sr for _, sr in seen], 1), want)


def test_one_axis_padded_while_the_other_is_tiled(cuda):
    """70 x 112 with tile (96, 64): the rows are one window of 70, padded to 72 by reflection; the columns are two tiles"""
    u8, want = _want(cuda, "x4", 1, 3, 70, 112, 34, (96, 64), 16, pad="reflect")
    net = _net(cuda)
    with torch.no_grad():
        got = net.forward_tiled(u8.to(cuda), (96, 64), overlap=16, pad="reflect")
        assert tuple(got.shape) == (1, 3, 3, 280, 448) and torch.equal(got, want)
        assert torch.equal(net.forward_tiled(u8.permute(0, 1, 3, 4, 2).contiguous(), (96, 64), overlap=16, pad="reflect"), want)
        with pytest.raises(ValueError):      # without `pad` the window's size is refused as the frame's would be
            net.forward_tiled(u8.to(cuda), (96, 64), overlap=16)


def test_the_x2_network_with_an_odd_window_start(cuda):
    """64 x 180, tile 64, overlap 15: windows at x0 = 0, 49, 98, 116 -- SR column 98 of the accumulator starts 8 bytes off a 16-byte
    boundary"""
    assert [x0 for _, _, x0, _ in R.plan_tiles(64, 180, 64, 15)] == [0, 49, 98, 116]
    u8, want = _want(cuda, "x2", 1, 2, 64, 180, 35, 64, 15)
    with torch.no_grad():
        got = _net(cuda, "x2").forward_tiled(u8.to(cuda), 64, overlap=15)
        assert tuple(got.shape) == (1, 2, 3, 128, 360) and torch.equal(got, want)


def test_refusals_come_before_any_launch(cuda):
    from eavsr_amd import harness, ops
    net = _net(cuda)
    x = _clip_u8(1, 2, 96, 112, 31).to(cuda)
    with torch.no_grad():
        refused = [lambda: net.forward_tiled(x, 60), lambda: net.forward_tiled(x, 66), lambda: net.forward_tiled(x, 64, overlap=33),
                   lambda: net.forward_tiled(x, 64, overlap=-1), lambda: net.forward_tiled(x, (64, 32)), lambda: net.forward_tiled(x, None),
                   lambda: net.forward_tiled(x, 64, pad="wrap"), lambda: net.forward_tiled(x, 64, segments=[(0, 1, 0, 1)]),
                   lambda: net.forward_tiled(x, 64, frame_chunk=0), lambda: net.forward_long(x, window=(0, 64, 60, 124)),
                   lambda: harness.super_resolve(net, x[0], tile=66), lambda: harness.super_resolve(net, x[0], tile=64, tile_overlap=40)]
        for i, fn in enumerate(refused):
            out, launched = _launches(ops, fn)
            assert isinstance(out, ValueError) and launched == {}, (i, out, launched)


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


def test_super_resolve_of_96x112_png_files_in_tiles(cuda, tmp_path, monkeypatch):
    from eavsr_amd import harness, ops
    from eavsr_amd.lpips import LPIPSAlex
    from tests import lpips_ref
    for name in ("EAVSR_TILE", "EAVSR_TILE_OVERLAP", "EAVSR_PAD_FRAMES"):
        monkeypatch.delenv(name, raising=False)
    lp = LPIPSAlex()
    lp.load_state_dict(lpips_ref.synthetic_weights(0), strict=True)
    lp = lp.to(cuda)
    model = _wrapper()
    u8, _ = _want(cuda, "x4", 1, 3, 96, 112, 31, 64, 16)
    with torch.no_grad():
        want = model.netEAVSRP.forward_tiled(u8.to(cuda), 64, overlap=32)      # super_resolve's default overlap
        want16 = model.netEAVSRP.forward_tiled(u8.to(cuda), 64, overlap=16)
    hr = _hr_for(u8[0])
    names = ["000_%05d.png" % i for i in range(3)]
    paths = [harness.write_png(u8[0, i], str(tmp_path / "lr" / names[i])) for i in range(3)]
    hr_paths = [harness.write_png(hr[i], str(tmp_path / "hr" / names[i])) for i in range(3)]
    tiles = R.plan_tiles(96, 112, 64, 32)

    def check(res, want=want, tiles=tiles, written=True):
        want_rgb8 = ops.rgb8(want[0], 255.0)
        want_metrics = harness.frame_metrics(want, ops.u8_to_f32(hr.to(cuda)).unsqueeze(0), 255.0, lpips=lp)
        assert res["frames"] == 3 and res["frame_names"] == names and [tuple(v) for v in res["tiles"]] == tiles
        assert res["frame_psnr"] == want_metrics["psnr"] and res["frame_ssim"] == want_metrics["ssim"]
        assert res["frame_lpips"] == want_metrics["lpips"]
        if written:
            assert [p.rsplit("/", 1)[1] for p in res["written"]] == names
            decoded = harness.decode_png_frames(res["written"], cuda, channels=3)
            assert tuple(decoded.shape) == (3, 3, 384, 448) and torch.equal(decoded.permute(0, 2, 3, 1), want_rgb8)

    for encoder in ("host", "device"):
        check(harness.super_resolve(model, paths, out_dir=str(tmp_path / encoder), hr=hr_paths, lpips=lp, tile=64, png_encoder=encoder,
                                    png_decoder="device"))
    check(harness.super_resolve(model, paths, hr=hr_paths, lpips=lp, tile="64x64", tile_overlap=16, frame_chunk=2), want=want16,
          tiles=R.plan_tiles(96, 112, 64, 16), written=False)
    # with segments: one window of frames here, the tiled path all the same
    res = harness.super_resolve(model, paths, hr=hr_paths, lpips=lp, tile=64, cuts="device", png_decoder="device")
    assert [tuple(seg) for seg in res["segments"]] == [(0, 3, 0, 3)]
    check(res, written=False)
    # not tiled: one window, and today's result
    plain = harness.super_resolve(model, paths, hr=hr_paths, lpips=lp)
    assert [tuple(v) for v in plain["tiles"]] == [(0, 96, 0, 112)] and plain["frame_psnr"] != res["frame_psnr"]
    # the environment alone, the options alone, and the options over the environment
    monkeypatch.setenv("EAVSR_TILE", "64")
    check(harness.super_resolve(model, paths, hr=hr_paths, lpips=lp, png_decoder="device"), written=False)
    check(harness.super_resolve(model.netEAVSRP, u8[0], hr=hr, lpips=lp, names=names), written=False)
    monkeypatch.setenv("EAVSR_TILE_OVERLAP", "16")
    check(harness.super_resolve(model, paths, hr=hr_paths, lpips=lp), want=want16, tiles=R.plan_tiles(96, 112, 64, 16), written=False)
    monkeypatch.setenv("EAVSR_TILE", "128")
    model.opt.tile, model.opt.tile_overlap = "64x64", 32
    check(harness.super_resolve(model, paths, hr=hr_paths, lpips=lp), written=False)


def test_evaluate_with_opt_tile(cuda, monkeypatch):
    from eavsr_amd import harness
    for name in ("EAVSR_TILE", "EAVSR_TILE_OVERLAP", "EAVSR_PAD_FRAMES"):
        monkeypatch.delenv(name, raising=False)
    u8, want = _want(cuda, "x4", 1, 3, 96, 112, 31, 64, 16)
    lr = torch.from_numpy(np.float32(u8.numpy()) / np.float32(255))
    hr = (_hr_for(u8[0]).float() / 255).unsqueeze(0)
    names = ["000_%05d.png" % i for i in range(3)]
    item = {"lr_seq": lr, "hr_seq": hr, "fname": names}
    model = _wrapper(tile=64, tile_overlap=16)
    rep = harness.evaluate(model, [item], per_frame=True, calc_ssim_flag=True)
    assert tuple(model.data_sr_seq.shape) == (1, 3, 3, 384, 448) and torch.equal(model.data_sr_seq, want)
    fm = harness.frame_metrics(want, hr.to(cuda), 255.0)
    assert rep["frame_psnr"] == fm["psnr"] and rep["frame_ssim"] == fm["ssim"] and rep["frame_names"] == names
    plain = _wrapper()
    harness.evaluate(plain, [item])
    assert not torch.equal(plain.data_sr_seq, want)
    default_overlap = _wrapper(tile="64")
    assert default_overlap.tile == (64, 64) and default_overlap.tile_overlap == 32
