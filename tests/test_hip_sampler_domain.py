"""Every bilinear sampler against the float64 references of the sampler-domain contract ("Sampler domain";
tests/sampler_domain.py): positions on the image edges, on the seams of the DCNv2 kernels' LDS windows, and wild ones -- huge,
infinite, NaN.  The tiers are separate cases: `-k "not wild"` runs the finite positions in or near the image, `-k wild` the rest.
The nine-product NCHW kernel (bf16x9) and the wave-specialised schedule (ws) exist in the lab build only: on the product library
their cases skip, as everywhere in this suite (tests/conftest.py); EAVSR_LIB_PATH=<lab library> runs them."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import sampler_domain as SD
from tests.golden import cases

pytestmark = pytest.mark.gpu

DCN_SHAPES = [(1, 64, 17, 70, 64, 8), (1, 16, 9, 33, 32, 2), (1, 48, 12, 20, 32, 2), (1, 64, 10, 12, 64, 1)]
X9_SHAPE = (1, 64, 17, 72, 64, 8)      # the nine-product NCHW kernel needs w % 4 == 0: the 3 x 3 ragged tiles again, at a width it takes
WARP_SHAPES = [(1, 8, 9, 70), (2, 3, 6, 10)]
DCN_TIERS = ["edge", "seam", "wild"]
EPS16 = {"bf16": 8e-3, "fp16": 1e-3}      # tests/test_hip_h16.py::test_dcnv2_il16_vs_oracle_on_rounded_operands


@pytest.fixture(scope="module")
def ops(cuda):
    from eavsr_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(params=["il2", "il", "ws"])
def il_impl(request, ops):
    prev = ops.DCN_IL_IMPL
    ops.set_dcn_il_impl(request.param)
    yield request.param
    ops.set_dcn_il_impl(prev)


def t(a, dev=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x if dev is None else x.to(dev)


def _pixels(h, w):
    """pixels whose every tap is made invalid: a tile corner, tile-interior pixels, the last pixel"""
    return sorted({(0, 0), (h // 2, w // 3), (h - 1, w - 1), (min(7, h - 1), min(31, w - 1)), (min(8, h - 1), min(32, w - 1))})


@functools.lru_cache(maxsize=None)
def dcn_case(shape, tier):
    """inputs (numpy, read-only) and the float64 reference, computed once per (shape, tier)"""
    n, c, h, w, cout, dg = shape
    rng = np.random.RandomState(7)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    mask = rng.uniform(0.1, 1.0, (n, dg * 9, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, c, 3, 3)) / (c * 9) ** 0.5).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1 + 0.05).astype(np.float32)
    off, _ = SD.dcn_offsets(tier, n, dg, h, w)
    if tier == "wild":
        off = SD.dcn_all_invalid(off, h, w, _pixels(h, w))
    ref = SD.dcnv2(x, off, mask, wt, b, dg)
    assert np.isfinite(ref).all()
    for a in (x, off, mask, wt, b, ref):
        a.setflags(write=False)
    return x, off, mask, wt, b, ref


def check_dcn(out, shape, tier, tol=3e-5):
    x, off, mask, wt, b, ref = dcn_case(shape, tier)
    out = out.double().cpu().numpy()
    err = np.abs(out - ref)
    bound = tol * max(1.0, np.abs(ref).max())
    print(f"dcn {shape} {tier}: max err {np.nan_to_num(err, nan=np.inf).max():.3e} (bound {bound:.3e}), non-finite outputs {(~np.isfinite(out)).sum()}")
    assert np.isfinite(out).all(), "a wild position poisoned the output"
    assert err.max() <= bound
    if tier == "wild" and tol == 3e-5:      # every tap invalid: the bias, bit for bit
        for (y, xx) in _pixels(shape[2], shape[3]):
            assert np.array_equal(out[0, :, y, xx].astype(np.float32).view(np.uint32), b.view(np.uint32)), (y, xx)


@pytest.mark.parametrize("tier", DCN_TIERS)
@pytest.mark.parametrize("mode", ["native", "bf16x9", "il6", "il9"])
@pytest.mark.parametrize("shape", DCN_SHAPES + [X9_SHAPE], ids=str)
def test_dcnv2_routes(ops, cuda, shape, mode, tier):
    """ops.modulated_deform_conv2d under every DCN mode: the NCHW kernel (native; (1, 48, 12, 20, 32, 2) whatever the mode), the
    nine-product NCHW kernel, the IL8 kernel under the default schedule"""
    x, off, mask, wt, b, _ = dcn_case(shape, tier)
    ops.set_dcn_mode(mode)
    with ops.profile() as prof:
        out = ops.modulated_deform_conv2d(t(x, cuda), t(off, cuda), t(mask, cuda), t(wt, cuda), t(b, cuda), 1, 1, 1, 1, shape[5])
    # the kernel the mode promises, not a fallback: an octet count that is no power of two goes to an NCHW kernel whatever the mode,
    # the nine-product kernel wants w % 4 == 0 (tests/test_hip_ops.py::test_dcnv2_x9_falls_back_to_native_kernel_on_unaligned_width)
    octets = shape[1] // shape[5] // 8
    if mode in ("il6", "il9") and octets & (octets - 1) == 0:
        want = "dcnv2_il"
    else:
        want = "dcnv2_x9" if mode == "bf16x9" and shape[3] % 4 == 0 else "dcnv2"
    assert [k for k in prof.summary() if k.startswith("dcnv2")] == [want], list(prof.summary())
    check_dcn(out, shape, tier)


@pytest.mark.parametrize("tier", DCN_TIERS)
def test_dcnv2_generic_kernel(ops, cuda, tier):
    """six channels per deformable group: no fused kernel takes it, eavsr_dcnv2_generic_f32 does"""
    shape = (1, 12, 9, 33, 8, 2)
    x, off, mask, wt, b, _ = dcn_case(shape, tier)
    with ops.profile() as prof:
        out = ops.modulated_deform_conv2d(t(x, cuda), t(off, cuda), t(mask, cuda), t(wt, cuda), t(b, cuda), 1, 1, 1, 1, 2)
    assert list(prof.summary()) == ["dcnv2_generic"], list(prof.summary())
    check_dcn(out, shape, tier)


@pytest.mark.parametrize("tier", DCN_TIERS)
@pytest.mark.parametrize("nprod", [6, 9])
@pytest.mark.parametrize("shape", [s for s in DCN_SHAPES if s[1] % 8 == 0 and (s[1] // s[5]) % 8 == 0 and s != DCN_SHAPES[2]], ids=str)
def test_dcnv2_il_schedules(ops, cuda, shape, nprod, tier, il_impl):
    x, off, mask, wt, b, _ = dcn_case(shape, tier)
    out = ops.dcnv2_il(ops.to_il8(t(x, cuda)), t(off, cuda), t(mask, cuda), t(wt, cuda), t(b, cuda), shape[5], nprod=nprod)
    check_dcn(out, shape, tier)


@pytest.mark.parametrize("tier", DCN_TIERS)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [DCN_SHAPES[0], DCN_SHAPES[1]], ids=str)
def test_dcnv2_il16(ops, cuda, shape, dt, tier):
    """the 16-bit kernel against the reference fed the same 16-bit-rounded features and weights"""
    x, off, mask, wt, b, _ = dcn_case(shape, tier)
    DT = {"bf16": torch.bfloat16, "fp16": torch.float16}[dt]
    xr, wr = t(x).to(DT).float().numpy(), t(wt).to(DT).float().numpy()
    ref = SD.dcnv2(xr, off, mask, wr, b, shape[5])
    out = ops.dcnv2_il16(ops.to_il8_h16(t(x, cuda), dt), t(off, cuda), t(mask, cuda), t(wt, cuda), t(b, cuda), shape[5]).double().cpu().numpy()
    assert np.isfinite(out).all()
    rel = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
    print(f"il16 {dt} {shape} {tier}: rel {rel:.3e}")
    assert rel <= EPS16[dt], rel
    if tier == "wild":
        for (y, xx) in _pixels(shape[2], shape[3]):
            assert np.array_equal(out[0, :, y, xx].astype(np.float32).view(np.uint32), b.view(np.uint32)), (y, xx)


def _heads_case(n, h, w, D, tier):
    rng = np.random.RandomState(21)
    heads = np.concatenate([rng.standard_normal((n, 4 * D, h, w)) * 0.4 + np.tile([1.0, 0, 0, 1.0], D).reshape(1, 4 * D, 1, 1),
                            rng.standard_normal((n, 2 * D, h, w)) * 1.5, rng.standard_normal((n, 9 * D, h, w)) * 2.0], 1).astype(np.float32)
    if tier == "wild":      # finite heads whose affine expansion overflows; one non-finite head (NaN offsets: inf x 0)
        idx = np.arange(h * w).reshape(h, w)
        for g in range(D):
            big = (idx * 7 + g) % 23 == 0
            heads[:, 4 * g + (g % 4), big] = 3e38 * (1 if g % 2 else -1)
            heads[:, 4 * g + ((g + 1) % 4), big] = 3e38 * (1 if g % 2 else -1)
            heads[:, 4 * D + 2 * g + (g % 2), (idx * 5 + g) % 29 == 0] = -3e38 if g % 3 else 2.0 ** 31
        heads[:, 0, h // 2, w // 2] = np.inf
        heads[:, 4 * D + 1, 1, 1] = np.nan
    return heads


@pytest.mark.parametrize("tier", ["ordinary", "edge", "seam", "wild"])
@pytest.mark.parametrize("nprod", [6, 9])
def test_dcnv2_heads_mode(ops, cuda, nprod, tier, il_impl):
    """heads mode: the offset is (T . R) - R + t in fp32 inside the kernel.  edge / seam: T = identity and t = a table offset, so the
    table's positions are reached through that formula.  wild: finite heads of order 1e38 overflow to +-inf offsets (T0 ry + T1 rx at
    the diagonal taps, t = -3e38) -- and ONLY to +-inf: ry, rx are -1, 0 or 1, every product is exact and finite, and a sum of finite
    terms that overflows cannot meet an opposite infinity, so no finite heads give a NaN offset; the NaN offsets of this case come
    from its two non-finite heads (inf x 0 and a NaN translation).  What a kernel makes of an infinite position -- the fraction
    inf - inf = NaN -- IS reached from finite heads.  The 16-bit kernel runs the same heads (once, under the default schedule)."""
    n, h, w, D = 1, 17, 70, 8
    c = 8 * D
    rng = np.random.RandomState(22)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    wt = (rng.standard_normal((64, c, 3, 3)) / (c * 9) ** 0.5).astype(np.float32)
    b = (rng.standard_normal(64) * 0.1).astype(np.float32)
    if tier in ("edge", "seam"):
        heads, _ = SD.heads_from_offsets(*SD.dcn_offsets(tier, n, D, h, w), D)
    else:
        heads = _heads_case(n, h, w, D, tier)
    off, m = SD.heads_offsets(heads, D)
    if tier == "wild":
        assert np.isinf(off).any() and np.isnan(off).any() and np.isfinite(off).mean() > 0.6
    ref = SD.dcnv2(x, off, m, wt, b, D)
    assert np.isfinite(ref).all()
    out = ops.dcnv2_il(ops.to_il8(t(x, cuda)), t(heads, cuda), None, t(wt, cuda), t(b, cuda), D, nprod=nprod, heads=True).double().cpu().numpy()
    assert np.isfinite(out).all()
    err = np.abs(out - ref).max()
    print(f"heads {tier} nprod {nprod}: err {err:.3e}")
    assert err <= 3e-5 * max(1.0, np.abs(ref).max())
    if il_impl == "il2" and nprod == 6:
        for dt, DT in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            ref16 = SD.dcnv2(t(x).to(DT).float().numpy(), off, m, t(wt).to(DT).float().numpy(), b, D)
            o16 = ops.dcnv2_il16(ops.to_il8_h16(t(x, cuda), dt), t(heads, cuda), None, t(wt, cuda), t(b, cuda), D, heads=True)
            o16 = o16.double().cpu().numpy()
            assert np.isfinite(o16).all(), dt
            rel = np.abs(o16 - ref16).max() / max(1.0, np.abs(ref16).max())
            print(f"heads il16 {dt} {tier}: rel {rel:.3e}")
            assert rel <= EPS16[dt], (dt, rel)


def _il8_shape(name):
    x, _, _, _, _, dg = cases.g4_inputs(name)
    return x.shape[1] % 8 == 0 and (x.shape[1] // dg) % 8 == 0


@pytest.mark.parametrize("name", [k for k in cases.G4_CASES if _il8_shape(k)])
def test_g4_known_answers_under_every_schedule_and_the_16_bit_kernel(ops, cuda, name, il_impl):
    gold = H.golden("g4_dcnv2")[name]
    x, off, mask, wt, b, dg = cases.g4_inputs(name)
    g = lambda v: v.to(cuda).contiguous()
    out = ops.dcnv2_il(ops.to_il8(g(x)), g(off), g(mask), g(wt), g(b), dg, nprod=9).cpu()
    assert H.maxabs(out, gold) <= 3e-5 * max(1.0, gold.abs().max().item())
    if il_impl == "il2":      # (the 16-bit kernel has one schedule)
        from oracle import eavsr_oracle as O
        for dt, DT in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            ref = O.dcnv2(x.to(DT).float(), off, mask, wt.to(DT).float(), b, 1, 1, 1, 1, dg)
            o16 = ops.dcnv2_il16(ops.to_il8_h16(g(x), dt), g(off), g(mask), g(wt), g(b), dg).cpu()
            assert H.maxabs(o16, ref) / max(1.0, ref.abs().max().item()) <= EPS16[dt], dt


# ---- flow_warp -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def warp_case(shape, tier, with_flow2):
    n, c, h, w = shape
    rng = np.random.RandomState(31)
    x = (rng.standard_normal((n, c, h, w)) - 0.3).astype(np.float32)
    flow, _ = SD.warp_flow(tier, n, h, w)
    if tier == "wild":
        flow = SD.warp_all_invalid(flow, _pixels(h, w))
    flow2 = (rng.standard_normal((n, 2, h, w)) * 0.5).astype(np.float32) if with_flow2 else None
    return x, flow, flow2


def check_warp(out, x, flow, flow2, pad, interp="bilinear", tier="edge"):
    ref, pinned = SD.flow_warp(x, flow, pad, flow2, interp)
    out = out.double().cpu().numpy()
    sel = np.broadcast_to(pinned[:, None], ref.shape)
    assert np.isfinite(out[sel]).all()
    err = np.abs(out - ref)[sel].max()
    print(f"warp {x.shape} {pad} {interp} {tier}: err {err:.3e}, unpinned pixels {(~pinned).sum()}")
    assert err <= 2e-5 * max(1.0, np.abs(x).max())
    if pad == "zeros" and tier == "wild" and flow2 is None:      # no valid corner: +0.0, sign included
        h, w = x.shape[2:]
        for (y, xx) in _pixels(h, w):
            assert (out[:, :, y, xx].astype(np.float32).view(np.uint32) == 0).all(), (y, xx)


@pytest.mark.parametrize("tier", ["edge", "wild"])
@pytest.mark.parametrize("with_flow2", [False, True])
@pytest.mark.parametrize("pad", ["zeros", "border"])
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=str)
def test_flow_warp_entry_points(ops, cuda, shape, pad, with_flow2, tier):
    """flow_warp, flow_warp_pair (NCHW and IL8 second output) and flow_warp_single against the reference, and against each other bit
    for bit -- on every pixel, the ones whose value the contract leaves open included"""
    x, flow, flow2 = warp_case(shape, tier, with_flow2)
    xb = np.ascontiguousarray(x[:, ::-1] * 0.5)
    g = lambda a: None if a is None else t(a, cuda)
    plain = ops.flow_warp(g(x), g(flow), padding_mode=pad, flow2=g(flow2))
    check_warp(plain, x, flow, flow2, pad, tier=tier)
    nhwc = ops.flow_warp(g(x), g(flow).permute(0, 2, 3, 1).contiguous(), padding_mode=pad, flow_layout="nhwc",
                         flow2=None if flow2 is None else g(flow2).permute(0, 2, 3, 1).contiguous())
    pa, pb = ops.flow_warp_pair(g(x), g(xb), g(flow), flow2=g(flow2), padding_mode=pad)
    sa = ops.flow_warp_single(g(x), g(flow), flow2=g(flow2), padding_mode=pad)
    check_warp(pb, xb, flow, flow2, pad, tier=tier)
    bits = lambda v: v.cpu().numpy().view(np.uint32)
    for name, other in (("nhwc", nhwc), ("pair", pa), ("single", sa)):
        assert np.array_equal(bits(plain), bits(other)), name
    if shape[1] % 8 == 0:
        _, pil = ops.flow_warp_pair(g(x), g(xb), g(flow), flow2=g(flow2), b_il8=True, padding_mode=pad)
        sil = ops.flow_warp_single(g(xb), g(flow), flow2=g(flow2), il8=True, padding_mode=pad)
        n, c, h, w = shape
        back = pil.permute(0, 1, 4, 2, 3).reshape(n, c, h, w).contiguous()
        assert np.array_equal(bits(back), bits(pb)) and np.array_equal(bits(pil), bits(sil))


@pytest.mark.parametrize("mode", [("reflection", "bilinear"), ("zeros", "nearest"), ("border", "nearest"), ("reflection", "nearest")])
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=str)
def test_flow_warp_reflection_and_nearest_on_the_edge_tier(ops, cuda, shape, mode):
    pad, interp = mode
    x, flow, flow2 = warp_case(shape, "edge", True)
    out = ops.flow_warp(t(x, cuda), t(flow, cuda), padding_mode=pad, flow2=t(flow2, cuda), interpolation=interp)
    check_warp(out, x, flow, flow2, pad, interp)


@pytest.mark.parametrize("tier", ["edge", "wild"])
@pytest.mark.parametrize("fs", [1, 2])
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=str)
def test_pwc_backwarp(ops, cuda, shape, fs, tier):
    """out and mask against the reference, either rounding of ((g + 1) size - 1) accepted per pixel; the mask is 0 and the output
    finite (0) at a non-finite position; summed corner weights on either side of 0.999 (edge tier)"""
    n, c, fh, fw = shape
    h, w = fh * fs, fw * fs
    rng = np.random.RandomState(41)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    flow = SD.pwc_flow(tier, n, h, w, fs)
    (o1, m1, ones1), (o2, m2, ones2) = SD.pwc_backwarp(x, flow, fs)
    out, mask = ops.pwc_backwarp(t(x, cuda), t(flow, cuda), with_mask=True)
    out_nomask = ops.pwc_backwarp(t(x, cuda), t(flow, cuda))
    assert torch.equal(out, out_nomask)
    out, mask = out.double().cpu().numpy(), mask.double().cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(mask).all()
    sure = ((np.abs(ones1 - 0.999) > 1e-5) & (np.abs(ones2 - 0.999) > 1e-5))[:, None]      # fp32 sum of the weights vs float64
    assert sure.mean() > 0.99
    assert (((mask == m1) | (mask == m2)) | ~sure).all()
    err = np.minimum(np.abs(out - o1), np.abs(out - o2))
    err = np.where(np.broadcast_to(sure, err.shape), err, 0)
    print(f"pwc {shape} fs {fs} {tier}: err {err.max():.3e}")
    assert err.max() <= 2e-5 * max(1.0, np.abs(x).max())
    for iy, ix in SD.pwc_positions(flow, h, w, fs):
        bad = ~(np.isfinite(iy) & np.isfinite(ix))
        assert (mask[:, 0][bad] == 0).all() and (out[np.broadcast_to(bad[:, None], out.shape)] == 0).all()


# ---- backward ------------------------------------------------------------------------------------------------------------------
def _check_grad(name, got, want, sel=None, tol=1e-4):
    got = got.double().cpu().numpy()
    assert np.isfinite(got).all(), name
    err = np.abs(got - want)
    if sel is not None:
        err = np.where(sel, err, 0)
    print(f"{name}: err {err.max():.3e} scale {np.abs(want).max():.3e}")
    assert err.max() <= tol * max(1.0, np.abs(want).max()), name


@pytest.mark.parametrize("tier", ["edge", "wild"])
@pytest.mark.parametrize("shape", WARP_SHAPES, ids=str)
def test_flow_warp_backward(ops, cuda, shape, tier):
    x, flow, _ = warp_case(shape, tier, False)
    g = np.random.RandomState(51).standard_normal(x.shape).astype(np.float32)
    dx_ref, dflow_ref, ok, anyin = SD.flow_warp_backward(x, flow, g)
    dx, dflow = ops.flow_warp_bwd(t(x, cuda), t(flow, cuda), None, t(g, cuda), True, True)
    dx_det = ops.flow_warp_bwd_dx_det(t(flow, cuda), None, t(g, cuda))
    _check_grad("dx", dx, dx_ref)
    _check_grad("dx_det", dx_det, dx_ref)
    _check_grad("dx vs det", dx, dx_det.double().cpu().numpy(), tol=2e-5)
    _check_grad("dflow", dflow, dflow_ref, ok)
    dead = np.broadcast_to(~anyin[:, None], dflow_ref.shape)      # no corner inside the image: exactly 0
    assert (dflow.cpu().numpy()[dead] == 0).all()


@functools.lru_cache(maxsize=None)
def dcn_bwd_case(shape, tier):
    x, off, mask, wt, b, _ = dcn_case(shape, tier)
    dy = np.random.RandomState(61).standard_normal((shape[0], shape[4], shape[2], shape[3])).astype(np.float32)
    return dy, SD.dcnv2_backward(x, off, mask, wt, dy, shape[5])


def _exact_zeros(shape, tier, doff, dmask):
    x, off, mask, wt, b, _ = dcn_case(shape, tier)
    n, c, h, w, cout, dg = shape
    py, px = SD.dcn_positions(off, dg)
    invalid = ~(SD.dcn_gate(py, px, h, w) & np.isfinite(py) & np.isfinite(px))
    assert invalid.any()
    assert (dmask.cpu().numpy().reshape(n, dg, 9, h, w)[invalid] == 0).all()
    assert (doff.cpu().numpy().reshape(n, dg, 9, 2, h, w)[np.broadcast_to(invalid[:, :, :, None], (n, dg, 9, 2, h, w))] == 0).all()


@pytest.mark.parametrize("tier", ["edge", "wild"])
def test_dcnv2_backward_sampler_path(ops, cuda, tier):
    shape = DCN_SHAPES[0]
    x, off, mask, wt, b, _ = dcn_case(shape, tier)
    dy, (dx_ref, doff_ref, dmask_ref, ok) = dcn_bwd_case(shape, tier)
    dx, doff, dmask, _ = ops.dcnv2_bwd(t(x, cuda), t(off, cuda), t(mask, cuda), t(wt, cuda), t(dy, cuda), 8)
    _check_grad("dx", dx, dx_ref)
    _check_grad("dmask", dmask, dmask_ref)
    _check_grad("doffset", doff, doff_ref, ok)
    _exact_zeros(shape, tier, doff, dmask)


@pytest.mark.parametrize("tier", ["edge", "wild"])
@pytest.mark.parametrize("shape", [DCN_SHAPES[0], DCN_SHAPES[1], DCN_SHAPES[2]], ids=str)
def test_dcnv2_backward_column_path(ops, cuda, shape, tier):
    """im2col against the reference's columns; col2im (atomic) and the deterministic dx against the reference's gradients"""
    x, off, mask, wt, b, _ = dcn_case(shape, tier)
    n, c, h, w, cout, dg = shape
    dy, (dx_ref, doff_ref, dmask_ref, ok) = dcn_bwd_case(shape, tier)
    col = ops.dcnv2_im2col(t(x, cuda), t(off, cuda), t(mask, cuda), dg)
    _check_grad("columns", col, SD.dcn_columns(x, off, mask, dg).reshape(n, c * 9, h, w), tol=2e-5)
    dcol = np.einsum("ok,nop->nkp", wt.reshape(cout, c * 9).astype(np.float64), dy.reshape(n, cout, h * w).astype(np.float64))
    dcol = dcol.reshape(n, c * 9, h, w).astype(np.float32)
    dx_ref, doff_ref, dmask_ref, ok = SD.dcnv2_backward(x, off, mask, wt, None, dg, dcol=dcol)
    dx, doff, dmask = ops.dcnv2_col2im(t(x, cuda), t(off, cuda), t(mask, cuda), t(dcol, cuda), dg)
    _check_grad("dx", dx, dx_ref)
    _check_grad("dmask", dmask, dmask_ref)
    _check_grad("doffset", doff, doff_ref, ok)
    _exact_zeros(shape, tier, doff, dmask)
    if (c, dg) == (64, 8):
        dx_det = ops.dcnv2_col2im_dx_det(t(off, cuda), t(mask, cuda), t(dcol, cuda), dg)
        _check_grad("dx_det", dx_det, dx_ref)
        _check_grad("dx vs det", dx, dx_det.double().cpu().numpy(), tol=2e-5)
