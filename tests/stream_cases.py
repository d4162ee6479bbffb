"""The table behind tests/test_hip_stream_order.py and tests/test_stream_cases_host.py: one row per public function of
`eavsr_amd.ops` that production code runs outside the default stream or that no whole-model graph test covers.  Not a test file.

A row's `make(seed, device)` returns a `Case`: the device buffers the op reads (for an in-place op: and writes), two complete sets
of VALID host values for them, A and B (in-range descriptors and indices, legal PNG filter bytes, finite floats: at no moment
does an op run on anything else), and the op's `out=` buffers.  `call(ops, bufs, outs)` runs the op on those buffers and
returns its output tensors.  Weights that the library caches in a derived form (LPIPS, PWC) are constants of the case, not
buffers: a captured launch reads the packed form the warm-up left, as `GraphedForward` documents.  `ref(A) -> wants` restates
the op on the host from tests/*_ref.py, `same(got, want)` compares with the bound the op's own test file uses (equality
unless it says otherwise).  `trim(outputs)` cuts outputs to the part the op defines (the streams of a `Deflated` buffer).

Shapes are the smallest that take every launch of an op: frames of 2 x 3 x 19 x 37 (rows that are no multiple of 4), more than
one workgroup partial where a second kernel sums partials (frame_metrics 37 x 83: two tiles; temporal_metrics 19 x 37: two;
lpips_tap 5 x 7: three), three unequal cache segments with an empty one, and `png_unfilter` on both sides of kLdsPixels.

The data comes from the case builders of the existing test files and tests/golden/cases.py."""
import os
import re
from typing import Callable, List, NamedTuple, Optional

import numpy as np
import torch

from tests import census_ref, ensemble_ref, pad_ref, png_ref, resample_ref, scene_ref, temporal_ref, tile_ref
from tests import helpers as H
from tests.golden import cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, C, FH, FW = 2, 3, 19, 37      # the frames of the ingest / blend / dihedral / metrics family


def lds_pixels() -> int:
    """kLdsPixels of csrc/png_decode.hip: rows wider than this take png_unfilter's allocating path"""
    with open(os.path.join(ROOT, "eavsr_amd", "csrc", "png_decode.hip")) as f:
        return int(re.search(r"constexpr\s+int\s+kLdsPixels\s*=\s*(\d+)\s*;", f.read()).group(1))


class Case(NamedTuple):
    bufs: List[torch.Tensor]
    A: List[torch.Tensor]
    B: List[torch.Tensor]
    outs: List[torch.Tensor] = []
    expect: Optional[list] = None      # the outputs for A where the builder knows them (the frames a PNG filter was applied to)


class Row(NamedTuple):
    name: str                 # the row's id
    op: str                   # the function of eavsr_amd.ops it runs
    make: Callable            # (seed, device) -> Case
    call: Callable            # (ops, bufs, outs) -> tuple of output tensors
    ref: Optional[Callable] = None      # (A as numpy arrays / tensors) -> tuple of expected outputs (None: not restated)
    same: Optional[Callable] = None     # (got, want) -> None or raises; default: equality
    trim: Optional[Callable] = None     # (outputs on the host) -> the defined part of them
    verify: Optional[Callable] = None   # (outputs for A on the host, A) -> None or raises: a check that is no comparison of tensors


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def _case(device, A, B, outs=()):
    A, B = [_t(a).contiguous() for a in A], [_t(b).contiguous() for b in B]
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(A, B))
    return Case([torch.empty(a.shape, dtype=a.dtype, device=device) for a in A], A, B, list(outs))


def _two(build, seed):
    """value sets A and B: the same builder at two seeds"""
    return build(seed), build(seed + 1000)


# ---------------------------------------------------------------------------------------------------- the builders of other files
def _pair(shape, seed):
    from tests.test_hip_metrics import make_pair
    return make_pair("noise", shape, seed)      # (sr, hr, 255.0)


def _source(layout, seed, f=F, c=C, h=FH, w=FW):
    from tests.test_hip_tile import _source as source
    x = source(layout, f, c, h, w, seed)
    if x.dtype == np.float32:      # (its three special bit patterns are for the bit-copying kernels' own tests: finite values here)
        x.reshape(-1)[:3] = (0.25, -1.5, 3.0)
    return x


def _png_frames(f, h, w, c, seed):
    from tests.test_hip_png import _frames
    return _frames(f, h, w, c, seed)


def _spread(count, seed, hi):
    from tests.test_hip_census import _spread as spread
    return spread(count, seed, lo=-30, hi=hi)


def _flows(seed, f=3, c=C, h=FH, w=FW):
    from tests.test_hip_temporal import _flow
    rng = np.random.default_rng(seed)
    seq = rng.random((f, c, h, w)).astype(np.float32)
    fw = _flow(rng, f, h, w, 0.7)
    bw = (-fw + rng.normal(0, 0.05, fw.shape)).astype(np.float32)
    return [seq, fw, bw, _flow(rng, f, h, w, 1.5)]


# ---------------------------------------------------------------------------------------------------- ingest, blend, ensemble
def _make_rgb8(seed, device):
    return _case(device, *_two(lambda s: [_pair((F, C, FH, FW), s)[0]], seed))


def _make_u8(layout):
    return lambda seed, device: _case(device, *_two(lambda s: [_source(layout, s)], seed))


PAD_H, PAD_W = 24, 44
WINDOW = (1, 3, 16, 30, 20, 36)      # y0, x0, wh, ww, H, W


def _make_blend(k):
    th, tw = 8, 13

    def make(seed, device):
        def build(s):
            sr_shape = (1, F, C, tw, th) if k & 4 else (1, F, C, th, tw)
            return [G.randn(s, 1, F, C, FH, FW), G.randn(s + 1, *sr_shape), G.rand(s + 2, th), G.rand(s + 3, tw)]
        return _case(device, *_two(build, seed))
    return make


BLEND_AT = (5, 7)      # Y0, X0


def _ref_blend(k):
    def ref(acc, sr, wy, wx):
        return (ensemble_ref.blend_oracle(acc.numpy().copy(), sr.numpy(), k, *BLEND_AT, wy.numpy(), wx.numpy()),)
    return ref


# ---------------------------------------------------------------------------------------------------- cache, scene, data set
SEGMENTS = ((1, 9001), (9002, 0), (9005, 333))      # (first element, count) in one flat buffer: unequal, one empty, none aligned
SEG_TOTAL = 9340


def _segments(flat):
    return [flat[a:a + n] for a, n in SEGMENTS]


def _make_pack16(census):
    def make(seed, device):
        A, B = _two(lambda s: [_spread(SEG_TOTAL, s, hi=18)] + ([np.zeros(5, np.int64)] if census else []), seed)
        return _case(device, A, B, [torch.empty(SEG_TOTAL + 3, dtype=torch.float16, device=device)])
    return make


def _dst16(out):
    return [out[a + 2:a + 2 + n] for a, n in SEGMENTS]      # another misalignment than the sources'


def _call_pack16(ops, b, o):
    return tuple(ops.pack16(_segments(b[0]), _dst16(o[0]), "fp16"))


def _call_pack16_census(ops, b, o):
    return tuple(ops.pack16_census(_segments(b[0]), _dst16(o[0]), "fp16", b[1])) + (b[1],)


def _ref_pack16(flat, *census):
    x = flat.numpy()
    segs = [x[a:a + n] for a, n in SEGMENTS]
    want = tuple(torch.from_numpy(census_ref.round16(s, "fp16").view(np.float16).copy()) for s in segs)
    if census:
        want += (torch.tensor(census_ref.row(census_ref.add(*[census_ref.census(s, "fp16") for s in segs])), dtype=torch.int64),)
    return want


def _same_bits(got, want):
    """16-bit floats by their bits: an overflow's inf compares, and so would a NaN"""
    if got.dtype in (torch.float16, torch.bfloat16):
        got, want = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    assert got.shape == want.shape and torch.equal(got, want)


def _make_unpack16(seed, device):
    A, B = _two(lambda s: [torch.from_numpy(_spread(SEG_TOTAL, s, hi=14)).to(torch.float16)], seed)      # finite in fp16
    return _case(device, A, B, [torch.empty(SEG_TOTAL + 3, dtype=torch.float32, device=device)])


def _make_frame_change(seed, device):
    from tests.test_hip_scene import _frames
    return _case(device, *_two(lambda s: [_frames((3, C, FH, FW), s)], seed))


PATCH, SCALE = 8, 2


def _make_gather(seed, device):
    from tests.test_hip_dataset import _stores

    def build(s):
        lr, hr = _stores(4, C, FH, FW, SCALE, s)
        k = s % 2      # two legal plans: windows inside the 19 x 37 frames, every flag, frames 0 .. 3
        frames = np.asarray([[0, 3], [2, 1], [1, 1]] if k else [[3, 0], [1, 2], [0, 0]], np.int32)
        desc = np.asarray([[0, 1, 5, 0], [11, 29, 2, 0], [3, 14, 7, 0]] if k else [[11, 0, 3, 0], [2, 27, 4, 0], [5, 6, 0, 0]], np.int32)
        return [lr, hr, frames, desc]
    A, B = build(seed), build(seed + 1)
    outs = [torch.empty((3, 2, C, PATCH, PATCH), device=device), torch.empty((3, 2, C, SCALE * PATCH, SCALE * PATCH), device=device)]
    return _case(device, A, B, outs)


def _ref_gather(lr, hr, frames, desc):
    f, d = frames.numpy(), desc.numpy()
    return (torch.from_numpy(H.restate_pairs(lr.numpy(), f, d, PATCH, PATCH)),
            torch.from_numpy(H.restate_pairs(hr.numpy(), f, d, PATCH, PATCH, SCALE)))


def _make_cubic(seed, device):
    from tests.test_hip_resample import _bytes
    A, B = _two(lambda s: [_bytes((F, C, 2 * FH, 2 * FW), s)], seed)
    return _case(device, A, B, [torch.empty((F, C, FH, FW), dtype=torch.uint8, device=device)])


# ---------------------------------------------------------------------------------------------------- PNG
def _make_png_frames(seed, device, out_shape=None):
    A, B = _two(lambda s: [_png_frames(F, FH, FW, C, s)], seed)
    return _case(device, A, B, [] if out_shape is None else [torch.empty(out_shape, dtype=torch.uint8, device=device)])


STRIPE_ROWS = 4
ROW_BYTES = 1 + FW * C


def _make_deflate(seed, device):
    return _case(device, *_two(lambda s: [png_ref.filter_frames(_png_frames(F, FH, FW, C, s)).reshape(F, FH * ROW_BYTES)], seed))


def _streams(outs):
    """a Deflated buffer is defined where its streams lie: (sizes, the streams end to end)"""
    data, offsets, sizes = outs
    return [sizes, offsets, torch.cat([data[int(o):int(o) + int(n)] for o, n in zip(offsets.tolist(), sizes.tolist())])]


def _make_unfilter(h, w):
    def make(seed, device):
        frames = _png_frames(F, h, w, C, seed)
        A, B = [png_ref.filter_frames(frames)], [png_ref.filter_frames(_png_frames(F, h, w, C, seed + 1000))]
        case = _case(device, A, B, [torch.empty((F, C, h, w), dtype=torch.uint8, device=device)])
        return case._replace(expect=[_t(frames.transpose(0, 3, 1, 2))])      # unfiltering gives back what was filtered
    return make


# ---------------------------------------------------------------------------------------------------- metrics
METRIC_SHAPE = (F, C, 37, 83)      # (83 - 10) / 64 -> two tiles per frame: the summing kernel adds two partials


def _make_frame_metrics(seed, device):
    return _case(device, *_two(lambda s: list(_pair(METRIC_SHAPE, s)[:2]), seed))


def _make_temporal(seed, device):
    return _case(device, *_two(_flows, seed))


def _ref_temporal(seq, fw, bw, flow_b):
    err, count, epe = temporal_ref.temporal_ref32(seq.numpy(), fw.numpy(), bw.numpy(), 255.0, flow_b.numpy())
    return torch.from_numpy(np.asarray(err, np.float64)), torch.from_numpy(np.asarray(count, np.int64)), torch.from_numpy(np.asarray(epe, np.float64))


def _same_temporal(got, want):
    """tests/test_hip_temporal.py: count is equal, the float64 sums agree to RTOL = 1e-10"""
    if got.dtype == torch.int64:
        assert torch.equal(got, want)
    else:
        assert got.shape == want.shape and ((got - want).abs() <= 1e-10 * want.abs()).all(), (got, want)


NIQE_BLOCK = 8
HALF_H, HALF_W = 24, 40


def _make_niqe_half(seed, device):
    from eavsr_amd import niqe, ops
    case = _case(device, *_two(lambda s: [G.rand(s, F, 1, HALF_H, HALF_W).double() * 255.0], seed))
    tables = ops.niqe_half_tables(niqe.resize_tables(HALF_H), niqe.resize_tables(HALF_W), device)
    torch.cuda.synchronize(device)      # uploaded here, on the default stream: a constant of the case
    return case._replace(bufs=case.bufs + [tables])


# ---------------------------------------------------------------------------------------------------- LPIPS and PWC
def _lpips_sd(device):
    from tests import lpips_ref
    sd = {k: v.to(device).contiguous() for k, v in lpips_ref.synthetic_weights(0).items()}
    torch.cuda.synchronize(device)
    return sd


def _with_consts(case, *consts):
    """constants ride behind the buffers; they have no A / B values and are never rewritten"""
    return case._replace(bufs=case.bufs + list(consts))


def _make_lpips_conv1(seed, device):
    from tests import lpips_ref
    sd = _lpips_sd(device)
    case = _case(device, *_two(lambda s: list(lpips_ref.image_pair(F, 35, 51, s)), seed))
    return _with_consts(case, sd["net.slice1.0.weight"], sd["net.slice1.0.bias"], sd["scaling_layer.shift"], sd["scaling_layer.scale"])


def _make_lpips_conv(seed, device):
    sd = _lpips_sd(device)
    case = _case(device, *_two(lambda s: [G.rand(s, F, 64, 5, 7)], seed))
    return _with_consts(case, sd["net.slice2.3.weight"], sd["net.slice2.3.bias"])


def _make_lpips_tap(seed, device):
    sd = _lpips_sd(device)
    case = _case(device, *_two(lambda s: [G.rand(s, 2 * F, 64, 5, 7)], seed))      # 35 pixels: three partials of 16 per frame
    return _with_consts(case, sd["lin0.model.1.weight"])


def _dev_consts(device, *tensors):
    out = [t.to(device).contiguous() for t in tensors]
    torch.cuda.synchronize(device)
    return out


def _make_pwc_conv(seed, device):
    case = _case(device, *_two(lambda s: [G.randn(s, F, 6, FH, FW)], seed))
    return _with_consts(case, *_dev_consts(device, G.randn(71, 8, 6, 3, 3, scale=0.1), G.randn(72, 8, scale=0.1)))


def _make_pwc_deconv(seed, device):
    case = _case(device, *_two(lambda s: [G.randn(s, F, 6, 9, 13)], seed))
    return _with_consts(case, *_dev_consts(device, G.randn(73, 6, 2, 4, 4, scale=0.1), G.randn(74, 2, scale=0.1)))


def _make_randn(*shapes, scale=1.0):
    return lambda seed, device: _case(device, *_two(lambda s: [G.randn(s + i, *shp, scale=scale) for i, shp in enumerate(shapes)], seed))


def _make_backwarp(seed, device):
    # (9 x 22 frames and flows of 0.6 px, the odd case of test_pwc_backwarp_decoder_mode: its absolute bound of 1e-5 against the
    #  normalised-grid restatement is for such inputs -- the restatement's own fp32 coordinate error grows with the frame width)
    return _case(device, *_two(lambda s: [G.randn(s, F, 4, 9, 22), G.randn(s + 1, F, 2, 9, 22, scale=0.6)], seed))


def _make_normalize(seed, device):
    case = _case(device, *_two(lambda s: [G.rand(s, F, C, FH, FW)], seed))
    return _with_consts(case, *_dev_consts(device, torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])))


def _np(fn):
    """a numpy restatement as a `ref`: tensors in, a tuple of tensors out"""
    def ref(*values):
        out = fn(*[v.numpy() for v in values])
        return tuple(_t(o) for o in (out if isinstance(out, tuple) else (out,)))
    return ref


def _ref_rgb8(sr):
    from tests.test_hip_metrics import quantised
    return (quantised(sr, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous(),)


def _verify_frame_metrics(got, A):
    from tests.test_hip_metrics import check_against_host
    check_against_host(A[0], A[1], 255.0, got[0], got[1], got[2], "stream_cases frame_metrics")


def _verify_deflated(raw_of):
    """every stream inflates to the bytes that went in (zlib is the judge, as in tests/test_hip_png.py)"""
    def verify(got, A):
        import zlib
        sizes, _, data = got
        raw, at = raw_of(A), 0
        for f, n in enumerate(sizes.tolist()):
            assert zlib.decompress(data[at:at + n].numpy().tobytes()) == raw[f].tobytes(), f"stream {f} does not inflate to its input"
            at += n
    return verify


def _lpips_bound(ref64, ref32):
    """tests/test_hip_lpips.py check_features: max|gpu - ref64| <= max(8 max|ref32 - ref64|, 2^-20 max|ref64|)"""
    return max(8 * (ref32.double() - ref64).abs().max().item(), 2.0 ** -20 * ref64.abs().max().item())


def _ref_lpips(fn):
    """(ref64, bound) packed as one tensor pair for `_same_lpips`: the restatement in float64 and in float32"""
    def ref(*values):
        from tests import lpips_ref
        sd = lpips_ref.synthetic_weights(0)
        r64, r32 = fn(lpips_ref, sd, torch.float64, *values), fn(lpips_ref, sd, torch.float32, *values)
        return ((r64, _lpips_bound(r64, r32)),)
    return ref


def _same_lpips(got, want):
    ref64, bound = want
    assert got.shape == ref64.shape and (got.double() - ref64).abs().max().item() <= bound


def _lpips_conv1_ref(R, sd, dt, sr, hr):
    return R.layer(R.front_end(torch.cat([sr, hr], 0), sd, 255.0, dt), sd, 0)


def _lpips_conv_ref(R, sd, dt, x):
    key = R.LAYERS[1][0]
    return torch.nn.functional.relu(torch.nn.functional.conv2d(x.to(dt), sd[key + ".weight"].to(dt), sd[key + ".bias"].to(dt), padding=2))


def _ref_correlation(a, b):
    from tests import pwc_ref
    return (torch.nn.functional.leaky_relu(pwc_ref.correlation(a.double(), b.double()), 0.1),)


def _same_1e5(got, want):
    """tests/test_hip_pwc.py: 1e-5 of the output scale"""
    assert got.shape == want.shape and (got.double() - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())


def _verify_niqe_moments(got, A):
    """tests/test_hip_niqe.py test_moments_equal_the_restatement: the luma plane is equal, the counts are equal, the sums agree to 1e-10"""
    from tests import niqe_ref
    from tests.test_hip_niqe import _ref_plane, _same_moments
    moments, luma = got
    h, w = FH // NIQE_BLOCK * NIQE_BLOCK, FW // NIQE_BLOCK * NIQE_BLOCK
    for i, img in enumerate(A[0].numpy()):
        plane = _ref_plane(img, 255.0, 0, 0, h, w)
        assert np.array_equal(luma[i, 0].numpy(), plane), i
        _same_moments(moments[i].numpy(), niqe_ref.plane_moments(plane, NIQE_BLOCK), i)


def _verify_niqe_half(got, A):
    """tests/test_hip_niqe.py test_half_equals_the_general_imresize: 1e-12"""
    from tests import niqe_ref
    for i, plane in enumerate(A[0].numpy()):
        assert np.abs(got[0][i, 0].numpy() - niqe_ref.imresize(plane[0], 0.5)).max() <= 1e-12, i


def _verify_lpips_tap(got, A):
    from tests import lpips_ref
    from tests.test_hip_lpips import check_frames
    x, lin = A[0], lpips_ref.synthetic_weights(0)["lin0.model.1.weight"]
    check_frames("stream_cases lpips_tap", got[0], lpips_ref.tap_distance(x[:F].double(), x[F:].double(), lin), lpips_ref.tap_distance(x[:F], x[F:], lin))


def _same_2e5(got, want):
    """tests/test_hip_pwc.py (convolutions): 2e-5 of the output scale"""
    assert got.shape == want.shape and (got.double() - want.double()).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())


def _ref_pwc_conv(x):
    w, b = G.randn(71, 8, 6, 3, 3, scale=0.1), G.randn(72, 8, scale=0.1)
    return (torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x, w, b, padding=1), 0.1),)


def _ref_pwc_deconv(x):
    return (torch.nn.functional.conv_transpose2d(x, G.randn(73, 6, 2, 4, 4, scale=0.1), G.randn(74, 2, scale=0.1), stride=2, padding=1),)


def _verify_backwarp(got, A):
    from tests.test_hip_pwc import _check_warp
    mask = _check_warp(got[0], got[1], A[0], A[1])
    assert 0 < float(mask.mean()) < 1


def _within(tol):
    """tests/test_hip_ops.py test_glue_either_side_of_the_path_matches_aten: an absolute bound"""
    def same(got, want):
        assert got.shape == want.shape and (got.double() - want.double()).abs().max().item() <= tol
    return same


def _ref_normalize(x):
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return ((x - mean) / std,)


def _ref_resize(x):
    want = torch.nn.functional.interpolate(x, size=(11, 23), mode="bilinear", align_corners=False)
    want[:, 0] *= 0.5
    want[:, 1] *= 0.6
    return (want,)


ROWS = [
    # ingest, blend, ensemble
    Row("rgb8", "rgb8", _make_rgb8, lambda ops, b, o: (ops.rgb8(b[0]),), _ref_rgb8),
    Row("u8_to_f32-planar", "u8_to_f32", _make_u8("u8_planes"), lambda ops, b, o: (ops.u8_to_f32(b[0], hwc=False),),
        _np(lambda x: pad_ref.pad_oracle(x, FH, FW, "edge"))),
    Row("u8_to_f32-hwc", "u8_to_f32", _make_u8("u8_interleaved"), lambda ops, b, o: (ops.u8_to_f32(b[0], hwc=True),),
        _np(lambda x: pad_ref.pad_oracle(x, FH, FW, "edge", hwc=True))),
    Row("ingest_pad", "ingest_pad", _make_u8("u8_planes"), lambda ops, b, o: (ops.ingest_pad(b[0], PAD_H, PAD_W, "reflect"),),
        _np(lambda x: pad_ref.pad_oracle(x, PAD_H, PAD_W, "reflect"))),
    Row("ingest_window", "ingest_window", _make_u8("u8_interleaved"),
        lambda ops, b, o: (ops.ingest_window(b[0], *WINDOW, mode="reflect", hwc=True),),
        _np(lambda x: tile_ref.window_oracle(x, *WINDOW, "reflect", hwc=True))),
    Row("tile_blend", "tile_blend", _make_blend(0), lambda ops, b, o: (ops.tile_blend(b[0], b[1], *BLEND_AT, b[2], b[3]),), _ref_blend(0)),
    Row("dihedral", "dihedral", _make_u8("f32_planes"), lambda ops, b, o: (ops.dihedral(b[0], 5),),
        _np(lambda x: np.ascontiguousarray(ensemble_ref.g(x, 5)))),
    Row("blend_dihedral-row", "blend_dihedral", _make_blend(3), lambda ops, b, o: (ops.blend_dihedral(b[0], b[1], 3, *BLEND_AT, b[2], b[3]),),
        _ref_blend(3)),
    Row("blend_dihedral-transposed", "blend_dihedral", _make_blend(5),
        lambda ops, b, o: (ops.blend_dihedral(b[0], b[1], 5, *BLEND_AT, b[2], b[3]),), _ref_blend(5)),
    # cache, scene, data set
    Row("pack16", "pack16", _make_pack16(False), _call_pack16, _ref_pack16, _same_bits),
    Row("pack16_census", "pack16_census", _make_pack16(True), _call_pack16_census, _ref_pack16, _same_bits),
    Row("unpack16", "unpack16", _make_unpack16, lambda ops, b, o: tuple(ops.unpack16(_segments(b[0]), [t for t in _dst16(o[0])])),
        lambda flat: tuple(seg.float() for seg in _segments(flat))),      # widening is exact: census_ref.round16 read backwards
    Row("frame_change", "frame_change", _make_frame_change, lambda ops, b, o: tuple(ops.frame_change(b[0], hwc=False)),
        _np(lambda x: scene_ref.frame_change(x, hwc=False))),
    Row("gather_pairs", "gather_pairs", _make_gather, lambda ops, b, o: tuple(ops.gather_pairs(b[0], b[1], b[2], b[3], PATCH, SCALE, out=(o[0], o[1]))),
        _ref_gather),
    Row("resize_cubic_u8", "resize_cubic_u8", _make_cubic, lambda ops, b, o: (ops.resize_cubic_u8(b[0], (FH, FW), out=o[0]),),
        _np(lambda x: resample_ref.resize_cubic_u8(x, (FH, FW))[0])),
    # PNG
    Row("png_filter", "png_filter", lambda s, d: _make_png_frames(s, d, (F, FH, ROW_BYTES)), lambda ops, b, o: (ops.png_filter(b[0], out=o[0]),),
        _np(png_ref.filter_frames)),
    Row("deflate_huffman", "deflate_huffman", _make_deflate, lambda ops, b, o: tuple(ops.deflate_huffman(b[0], STRIPE_ROWS * ROW_BYTES)),
        trim=_streams, verify=_verify_deflated(lambda A: A[0].numpy())),
    Row("png_encode", "png_encode", _make_png_frames, lambda ops, b, o: tuple(ops.png_encode(b[0], stripe_rows=STRIPE_ROWS)), trim=_streams,
        verify=_verify_deflated(lambda A: png_ref.filter_frames(A[0].numpy()).reshape(F, -1))),
    Row("png_unfilter-narrow", "png_unfilter", _make_unfilter(FH, FW), lambda ops, b, o: (ops.png_unfilter(b[0], C, out=o[0]),)),
    Row("png_unfilter-wide", "png_unfilter", _make_unfilter(3, lds_pixels() + 1), lambda ops, b, o: (ops.png_unfilter(b[0], C, out=o[0]),)),
    # metrics
    Row("frame_metrics", "frame_metrics", _make_frame_metrics, lambda ops, b, o: tuple(ops.frame_metrics(b[0], b[1], rgb8=True)),
        verify=_verify_frame_metrics),
    Row("temporal_metrics", "temporal_metrics", _make_temporal, lambda ops, b, o: tuple(ops.temporal_metrics(b[0], b[1], b[2], 255.0, b[3])),
        _ref_temporal, _same_temporal),
    Row("niqe_moments", "niqe_moments", _make_rgb8, lambda ops, b, o: tuple(ops.niqe_moments(b[0], block=NIQE_BLOCK)),
        verify=_verify_niqe_moments),
    Row("niqe_half", "niqe_half", _make_niqe_half, lambda ops, b, o: (ops.niqe_half(b[0], b[1]),), verify=_verify_niqe_half),
    # LPIPS and PWC
    Row("lpips_conv1", "lpips_conv1", _make_lpips_conv1, lambda ops, b, o: (ops.lpips_conv1(*b),), _ref_lpips(_lpips_conv1_ref), _same_lpips),
    Row("lpips_conv", "lpips_conv", _make_lpips_conv, lambda ops, b, o: (ops.lpips_conv(*b),), _ref_lpips(_lpips_conv_ref), _same_lpips),
    Row("lpips_maxpool", "lpips_maxpool", _make_randn((F, 5, 9, 11)), lambda ops, b, o: (ops.lpips_maxpool(b[0]),),
        lambda x: (torch.nn.functional.max_pool2d(x, 3, 2),)),      # compared for equality, as tests/test_hip_lpips.py does
    Row("lpips_tap", "lpips_tap", _make_lpips_tap, lambda ops, b, o: (ops.lpips_tap(b[0], b[1]),), verify=_verify_lpips_tap),
    Row("pwc_conv3x3", "pwc_conv3x3", _make_pwc_conv, lambda ops, b, o: (ops.pwc_conv3x3(*b),), _ref_pwc_conv, _same_2e5),
    Row("pwc_deconv4x4s2", "pwc_deconv4x4s2", _make_pwc_deconv, lambda ops, b, o: (ops.pwc_deconv4x4s2(*b),), _ref_pwc_deconv, _same_2e5),
    Row("pwc_correlation", "pwc_correlation", _make_randn((F, 8, 9, 13), (F, 8, 9, 13)), lambda ops, b, o: (ops.pwc_correlation(b[0], b[1]),),
        _ref_correlation, _same_1e5),
    Row("pwc_backwarp", "pwc_backwarp", _make_backwarp, lambda ops, b, o: tuple(ops.pwc_backwarp(b[0], b[1], with_mask=True)),
        verify=_verify_backwarp),
    # glue
    Row("normalize", "normalize", _make_normalize, lambda ops, b, o: (ops.normalize(*b),), _ref_normalize, _within(1e-6)),
    Row("avg_pool2", "avg_pool2", _make_randn((F, C, 18, 38)), lambda ops, b, o: (ops.avg_pool2(b[0]),),
        lambda x: (torch.nn.functional.avg_pool2d(x, 2, 2, count_include_pad=False),), _within(1e-6)),
    Row("resize_bilinear", "resize_bilinear", _make_randn((F, 2, FH, FW)), lambda ops, b, o: (ops.resize_bilinear(b[0], (11, 23), (0.5, 0.6)),),
        _ref_resize, _within(2e-6)),
    # (the 16-bit alignment's layout converter: inside the model the paired warp writes IL8 itself, so no graph test calls it)
    Row("to_il8_h16", "to_il8_h16", _make_randn((F, 24, 7, 9)), lambda ops, b, o: (ops.to_il8_h16(b[0], "bf16"),),
        lambda x: (x.view(F, 3, 8, 7, 9).permute(0, 1, 3, 4, 2).to(torch.bfloat16).contiguous(),)),      # tests/test_hip_h16.py's statement
    # selftest_mfma has no buffers and no value sets: parts (a) and (b) show nothing for it.  It has a row because it hands a stream to
    # the library (the host scan asks for a classification) and because it is the one such function that waits for the device by design.
    Row("selftest_mfma", "selftest_mfma", lambda seed, device: Case([], [], []),
        lambda ops, b, o: (torch.tensor(ops.selftest_mfma(torch.cuda.current_device())),)),
    Row("concat3", "concat3", _make_randn((F, 2, FH, FW), (F, 3, FH, FW), (F, 1, FH, FW)), lambda ops, b, o: (ops.concat3(*b),), lambda a, b, c: (torch.cat([a, b, c], 1),)),
]

# Rows whose op promises a host value in its docstring and therefore waits for the device by design: {row name: the phrase}.
# Every other row returns device tensors only ("nothing is read back, so the call does not wait for the device", `deflate_huffman`).
HOST_SYNC = {
    "selftest_mfma": 'returns a Python int: "Number of accumulator elements that disagree with the assumed MFMA lane layout (0 = OK)"',
}

# Rows left out of the capture test: {row name: why}.
NOT_CAPTURED = {
    "png_unfilter-wide": "rows wider than kLdsPixels take their hand-over row from hipMallocAsync / hipFreeAsync in stream order",
}

# Ops of the model's own forward and backward: {function: the whole-model graph test that runs the model it belongs to under
# capture}.
_FWD = "test_hip_graph_replay_reproduces_the_eager_forward"
_TRAIN = "test_graphed_training_step_matches_eager"
_DET = "test_training_steps_repeat_bit_for_bit"
_H16 = "test_graphed_forward_in_the_16bit_mode_reproduces_the_eager_forward"      # (asserts that it called each of them)
MODEL_OPS = {
    **{k: _FWD for k in ("flow_warp", "flow_warp_pair", "flow_warp_single", "conv2d", "modulated_deform_conv2d", "to_il8", "dcnv2_il",
                         "adapt_frontend", "affine_offsets", "resize_bilinear_ac", "pyramid", "add", "ca_scale", "ca_tail", "scale_residual",
                         "ca_scale_pre", "gconv3x3")},
    **{k: _TRAIN for k in ("prepack_conv3_x6", "act_bwd", "plane_sum", "channel_sum", "scale_residual_bwd", "ca_mlp_bwd", "rcab_tail_bwd",
                           "flow_warp_bwd", "resize_bilinear_ac_bwd", "pyramid_bwd", "affine_offsets_bwd", "conv_wgrad", "conv_wgrad_multi",
                           "channel_sum_multi", "dcnv2_bwd", "dcnv2_im2col", "dcnv2_col2im", "gconv3x3_bwd")},
    **{k: _DET for k in ("resize_bilinear_ac_bwd_det", "flow_warp_bwd_dx_det", "dcnv2_col2im_dx_det")},
    **{k: _H16 for k in ("dcnv2_il16", "to_nhwc_h16", "from_nhwc_h16", "conv3x3_c64_h16", "ca_scale_pre_h16",
                         "conv3x3_c64_h16_res", "conv3x3_c64_h16_act", "conv3x3_c64to3_h16", "conv5x5_c64_h16", "scale_residual_h16")},
}

# Functions that exist only in the lab build of the library (ops.require_lab at their top): {function: what it is}.
LAB_ONLY = {
    "flow_level": "one kernel per pyramid level",
    "rcab_convs_h16": "conv -> ReLU -> conv of a 16-bit RCAB as one launch",
}
