"""The training backward's glue kernels (csrc/backward.hip, backward_dcn.hip, dcn_bwd.hip) against CPU float64 autograd of the
plain operation (tests/backward_refs.py), at the training shapes and at the edges where such kernels go wrong: rows wider than one
64-wide block that end in a partial one, ragged planes, samples just outside the image or far outside it, degenerate sizes, every
gradient pattern the autograd wiring has.  Inputs are made in float64 and rounded to float32 once, so both sides see the same
operands.  Each gradient's bound is scaled by its own |ref|.max() (floor 1e-6); every test prints its worst relative error.
`pytest -m gpu -s`."""
import pytest
import torch

from tests import backward_refs as R

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
PIX = 2e-5        # per-pixel gradients: din, dx, dflow, dheads, gconv dx, forward outputs
RED = 1e-4        # reductions over pixels: gconv dweight / dbias, channel-attention MLP weights, DCN (all five gradients)


@pytest.fixture(scope="module")
def AG(cuda):
    from eavsr_amd import autograd as _ag, ops
    ops.lib()
    return _ag


def leaf(t64, dev=None, grad=True):
    """the float64 reference leaf (dev None) or its float32 GPU twin"""
    t = t64.clone() if dev is None else t64.float().to(dev)
    return t.requires_grad_(grad)


def vjp(out, G, inputs):
    """d(sum(out * G)) / d(inputs) for the inputs that require a gradient (None for the others)"""
    outs = out if isinstance(out, (tuple, list)) else (out,)
    Gs = G if isinstance(G, (tuple, list)) else (G,)
    loss = sum((o * g.to(o.device, o.dtype)).sum() for o, g in zip(outs, Gs) if o is not None)
    need = [t for t in inputs if t.requires_grad]
    got = iter(torch.autograd.grad(loss, need))
    return [next(got) if t.requires_grad else None for t in inputs]


def close(tag, pairs, tol):
    """pairs: name -> (gpu, float64 reference); tol: one bound or name -> bound, times max(|ref|.max(), FLOOR) per tensor.
    Prints every tensor's relative error (the figures the bounds were set from) before asserting."""
    errs = {}
    for name, (got, ref) in pairs.items():
        assert (got is None) == (ref is None), (tag, name, got is None, ref is None)
        if ref is None:
            continue
        ref = ref.detach().double().cpu()
        got = got.detach().double().cpu()
        assert got.shape == ref.shape, (tag, name, tuple(got.shape), tuple(ref.shape))
        errs[name] = (got - ref).abs().max().item() / max(ref.abs().max().item(), FLOOR)
    print(f"\n[{tag}] worst relative error: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, e in errs.items():
        bound = tol[name] if isinstance(tol, dict) else tol
        assert e <= bound, (tag, name, e, bound)


# ------------------------------------------------------------------------------------------ 1. resize_bilinear_ac
# (hin, win) -> (hout, wout), scale: the training directions (networks.py: x0.25 and x0.5 of the offset, x2 of the residual flows)
RESIZE = {
    "down4_96x96": ((96, 96), (24, 24), 0.25),
    "down2_96x96": ((96, 96), (48, 48), 0.5),
    "up2_24x24": ((24, 24), (48, 48), 2.0),
    "up2_48x48": ((48, 48), (96, 96), 2.0),
    "down4_52x132_ragged": ((52, 132), (13, 33), 0.25),
    "down2_52x132_ragged": ((52, 132), (26, 66), 0.5),
    "up2_26x66_ragged": ((26, 66), (52, 132), 2.0),
    "down4_4x132_hout1": ((4, 132), (1, 33), 0.25),
}


def _resize_case(AG, cuda, tag, n, c, hw_in, hw_out, scale, x_grad, pre_mode, post_mode, seed):
    x = R.randn64(seed, n, c, *hw_in)
    pre = None if pre_mode == "none" else R.randn64(seed + 1, n, c, *hw_in)
    post = None if post_mode == "none" else R.randn64(seed + 2, n, c, *hw_out)
    G = R.randn64(seed + 3, n, c, *hw_out)
    grads = {"x": x_grad, "pre": pre_mode == "grad", "post": post_mode == "grad"}
    cl = [None if t is None else leaf(t, grad=grads[k]) for k, t in (("x", x), ("pre", pre), ("post", post))]
    gl = [None if t is None else leaf(t, cuda, grad=grads[k]) for k, t in (("x", x), ("pre", pre), ("post", post))]
    ref_out = R.resize_ac(cl[0], hw_out, scale, cl[1], cl[2])
    got_out = AG.resize_bilinear_ac(gl[0], hw_out, scale, pre_add=gl[1], post_add=gl[2])
    present = [t for t in cl if t is not None]
    ref = vjp(ref_out, G, present)
    got = vjp(got_out, G, [t for t in gl if t is not None])
    names = [k for k, t in zip(("x", "pre", "post"), cl) if t is not None]
    close(tag, {"out": (got_out, ref_out), **{f"d{k}": (g, r) for k, g, r in zip(names, got, ref)}}, PIX)


@pytest.mark.parametrize("c", [144, 2], ids=["c144", "c2"])
@pytest.mark.parametrize("case", list(RESIZE))
def test_resize_bilinear_ac_backward(AG, cuda, case, c):
    """din of every training direction and size, the ragged one (w > 64, odd output) and hout == 1 (rh = 0), with a gradient
    through pre_add and post_add as well"""
    hw_in, hw_out, scale = RESIZE[case]
    _resize_case(AG, cuda, f"resize {case} c{c}", 2, c, hw_in, hw_out, scale, True, "grad", "grad", 100 + c)


@pytest.mark.parametrize("post", ["none", "const", "grad"], ids=lambda s: f"post_{s}")
@pytest.mark.parametrize("pre", ["none", "const", "grad"], ids=lambda s: f"pre_{s}")
@pytest.mark.parametrize("case,c", [("down4_96x96", 144), ("up2_24x24", 2)], ids=["down4_96x96_c144", "up2_24x24_c2"])
def test_resize_bilinear_ac_backward_add_operands(AG, cuda, case, c, pre, post):
    """every combination of pre_add / post_add absent, present without a gradient and present with one"""
    hw_in, hw_out, scale = RESIZE[case]
    _resize_case(AG, cuda, f"resize {case} c{c} pre {pre} post {post}", 2, c, hw_in, hw_out, scale, True, pre, post, 200)


def test_resize_bilinear_ac_backward_through_pre_add_only(AG, cuda):
    """x without a gradient, pre_add with one: din is still computed (needs_input_grad[1])"""
    _resize_case(AG, cuda, "resize up2_24x24 c2 x const, pre grad", 2, 2, (24, 24), (48, 48), 2.0, False, "grad", "const", 300)


# ------------------------------------------------------------------------------------------ 2. flow_warp
WARP_SHAPES = {"2x96x96": (2, 96, 96), "1x33x130": (1, 33, 130), "2x45x77": (2, 45, 77)}
# which inputs need a gradient: x, flow, flow2 (flow2 present in the last pattern only)
WARP_PATTERNS = {"dx_only": (True, False, None), "dflow_only": (False, True, None), "dx_dflow": (True, True, None),
                 "dflow2_only": (False, False, True)}


def _warp(AG, cuda, tag, n, c, h, w, region, pattern, seed):
    gx_, gf_, gf2_ = WARP_PATTERNS[pattern]
    x = R.randn64(seed, n, c, h, w)
    flow = R.warp_flow(seed + 1, n, h, w, region)
    G = R.randn64(seed + 2, n, c, h, w)
    if gf2_ is None:
        cl = [leaf(x, grad=gx_), leaf(flow, grad=gf_)]
        gl = [leaf(x, cuda, grad=gx_), leaf(flow, cuda, grad=gf_)]
        ref = vjp(R.flow_warp(*cl), G, cl)
        got = vjp(AG.flow_warp(*gl), G, gl)
        names = ["dx", "dflow"]
    else:       # flow = f1 + f2 with only f2 trainable (the residual flow of networks.py's levels 2 and 1)
        f1 = R.randn64(seed + 3, n, 2, h, w, scale=2.0)
        f2 = (flow - f1).float().double()
        cl = [leaf(x, grad=False), leaf(f1, grad=False), leaf(f2)]
        gl = [leaf(x, cuda, grad=False), leaf(f1, cuda, grad=False), leaf(f2, cuda)]
        ref = vjp(R.flow_warp(cl[0], cl[1], cl[2]), G, cl)
        got = vjp(AG.flow_warp(gl[0], gl[1], flow2=gl[2]), G, gl)
        names = ["dx", "dflow", "dflow2"]
    close(tag, dict(zip(names, zip(got, ref))), PIX)
    return flow, dict(zip(names, got)), dict(zip(names, ref))


@pytest.mark.parametrize("c", [64, 12, 2], ids=lambda c: f"c{c}")
@pytest.mark.parametrize("shape", list(WARP_SHAPES))
@pytest.mark.parametrize("pattern", list(WARP_PATTERNS))
def test_flow_warp_backward(AG, cuda, pattern, shape, c):
    """the four gradient patterns of autograd.flow_warp (dflow_only: need_dx=False) over rows that cross a 64-wide block and end in
    a partial one, with c = 12 leaving some of the kernel's eight channel slices empty; positions from every region"""
    n, h, w = WARP_SHAPES[shape]
    _warp(AG, cuda, f"flow_warp {pattern} {shape} c{c} mixed", n, c, h, w, "mixed", pattern, 400 + c)


@pytest.mark.parametrize("shape", list(WARP_SHAPES))
@pytest.mark.parametrize("region", ["inside", "edge", "far"])
def test_flow_warp_backward_regions(AG, cuda, region, shape):
    """positions well inside; one pixel outside an edge (one corner column / row valid, x = w - 1 + u among them); beyond the
    clamp.  Structure as well as values: dflow is exactly zero where no corner is valid, dx exactly zero where no sample reaches"""
    n, h, w = WARP_SHAPES[shape]
    flow, got, ref = _warp(AG, cuda, f"flow_warp dx_dflow {shape} c12 {region}", n, 12, h, w, region, "dx_dflow", 500)
    dead = R.no_valid_corner(flow)
    if region == "inside":
        assert not dead.any()
    if region == "far":
        assert dead.all()
    dflow = got["dflow"].cpu()
    assert (dflow.permute(1, 0, 2, 3)[:, dead] == 0).all(), "d(flow) where every corner is invalid"
    assert (ref["dflow"].permute(1, 0, 2, 3)[:, dead] == 0).all()
    unreached = ~R.reached(flow)
    dx = got["dx"].cpu()
    assert (dx.permute(1, 0, 2, 3)[:, unreached] == 0).all(), "dx in pixels that no sample reaches"
    if region == "far":
        assert unreached.all() and (dx == 0).all()


# ------------------------------------------------------------------------------------------ 3. affine_offsets
AFFINE_SHAPES = {"2x96x96": (2, 96, 96), "1x45x77": (1, 45, 77)}


def _affine(AG, cuda, tag, n, h, w, D, with_mask, logit_range, seed):
    hc = 15 * D if with_mask else 6 * D
    heads = R.randn64(seed, n, hc, h, w)
    if logit_range is not None:
        heads[:, 6 * D:] = R.uniform64(seed + 1, -logit_range, logit_range, n, 9 * D, h, w)
    Go = R.randn64(seed + 2, n, 18 * D, h, w)
    Gm = R.randn64(seed + 3, n, 9 * D, h, w) if with_mask else None
    ch, gh = leaf(heads), leaf(heads, cuda)
    ref_o, ref_m = R.affine(ch, D, with_mask)
    if with_mask:
        got_o, got_m = AG.affine_offsets(gh, D, True)
        (ref,), (got,) = vjp((ref_o, ref_m), (Go, Gm), [ch]), vjp((got_o, got_m), (Go, Gm), [gh])
    else:
        got_o, got_m = AG.affine_offsets(gh, D, False)
        (ref,), (got,) = vjp(ref_o, Go, [ch]), vjp(got_o, Go, [gh])
    pairs = {"offset": (got_o, ref_o), "dheads[transform,translation]": (got[:, :6 * D], ref[:, :6 * D])}
    if with_mask:
        pairs["mask"] = (got_m, ref_m)
        pairs["dheads[mask logits]"] = (got[:, 6 * D:], ref[:, 6 * D:])
    close(tag, pairs, PIX)


@pytest.mark.parametrize("shape", list(AFFINE_SHAPES))
@pytest.mark.parametrize("D,with_mask", [(1, False), (8, True)], ids=["D1_nomask", "D8_mask"])
def test_affine_offsets_backward(AG, cuda, D, with_mask, shape):
    """D = 1 without mask (AdaptBlock2_3x3 -> TransOffsetworelu) and D = 8 with mask (AdaptBlockOffset), 96 x 96 and a ragged plane"""
    n, h, w = AFFINE_SHAPES[shape]
    _affine(AG, cuda, f"affine D{D} mask {with_mask} {shape}", n, h, w, D, with_mask, None, 600 + D)


def test_affine_offsets_backward_saturated_mask(AG, cuda):
    """mask logits over [-30, 30]: sigmoid saturates (s (1 - s) underflows to 0 in float32 at the ends, 1e-13 in float64)"""
    _affine(AG, cuda, "affine D8 mask saturated 1x45x77", 1, 45, 77, 8, True, 30.0, 650)


# ------------------------------------------------------------------------------------------ 4. gconv3x3
GCONV_SHAPES = {"2x96x96": (2, 96, 96), "1x45x77": (1, 45, 77), "3x5x3": (3, 5, 3)}
GCONV_COUT = {1: 128, 2: 64}      # adapt_frontend: depthwise 128 -> 128, then 128 -> 64 with two inputs per output


def _gconv_inputs(cpg, n, h, w, seed):
    cout = GCONV_COUT[cpg]
    x = R.randn64(seed, n, cout * cpg, h, w)
    wt = R.randn64(seed + 1, cout, cpg, 3, 3, scale=1.0 / 3.0)
    b = R.randn64(seed + 2, cout, scale=0.1)
    return x, wt, b


@pytest.mark.parametrize("act", [None, "lrelu"], ids=["noact", "lrelu"])
@pytest.mark.parametrize("shape", list(GCONV_SHAPES))
@pytest.mark.parametrize("cpg", [1, 2], ids=["cpg1", "cpg2"])
def test_gconv3x3_forward_backward(AG, cuda, cpg, shape, act):
    """out, dx, dweight, dbias through autograd's _GConvFn (adapt_frontend's training form): 96 x 96 (hw > 2048: both halves of the
    wgrad kernel's pass), 45 x 77 (h % 4 != 0, w > 64), 5 x 3 (planes smaller than the border)"""
    n, h, w = GCONV_SHAPES[shape]
    x, wt, b = _gconv_inputs(cpg, n, h, w, 700 + cpg)
    G = R.randn64(703, n, GCONV_COUT[cpg], h, w)
    cl = [leaf(t) for t in (x, wt, b)]
    ref_out = R.gconv(cl[0], cl[1], cl[2], act)
    if act == "lrelu":
        # where the pre-activation is within float32 rounding of 0, float32 may take the other slope: no cotangent there
        z = R.gconv(x, wt, b, None)
        G = torch.where(z.abs() < 1e-5 * z.abs().max(), torch.zeros_like(G), G)
    ref = vjp(ref_out, G, cl)
    gl = [leaf(t, cuda) for t in (x, wt, b)]
    got_out = AG._GConvFn.apply(gl[0], gl[1], gl[2], cpg, act, 0.2)
    got = vjp(got_out, G, gl)
    close(f"gconv3x3 cpg{cpg} {shape} {act}", {"out": (got_out, ref_out), "dx": (got[0], ref[0]), "dweight": (got[1], ref[1]),
                                               "dbias": (got[2], ref[2])}, {"out": PIX, "dx": PIX, "dweight": RED, "dbias": RED})


@pytest.mark.parametrize("cpg", [1, 2], ids=["cpg1", "cpg2"])
def test_gconv3x3_backward_accumulates_into_buffers(AG, cuda, cpg):
    """ops.gconv3x3_bwd(grads=bufs, accumulate=True) twice (grad_sink's path) adds both uses' dweight / dbias to what the buffers
    held; with cpg = 2 the second input channel's workgroup must leave the bias buffer alone"""
    from eavsr_amd import ops
    n, h, w = 2, 96, 96
    cout = GCONV_COUT[cpg]
    x, wt, _ = _gconv_inputs(cpg, n, h, w, 750)
    g1, g2 = R.randn64(753, n, cout, h, w), R.randn64(754, n, cout, h, w)
    dw0, db0 = R.randn64(755, cout, cpg, 3, 3), R.randn64(756, cout)
    refs = []
    for g in (g1, g2):
        cx, cw = leaf(x), leaf(wt)
        cb = leaf(torch.zeros(cout, dtype=R.F64))
        refs.append(vjp(R.gconv(cx, cw, cb, None), g, [cx, cw, cb]))
    bufs = (dw0.float().to(cuda), db0.float().to(cuda))
    xg, wg = x.float().to(cuda), wt.float().to(cuda)
    dxs = []
    for g in (g1, g2):
        dx, dw, db = ops.gconv3x3_bwd(g.float().to(cuda), xg, wg, cpg, grads=bufs, accumulate=True)
        assert dw is bufs[0] and db is bufs[1]
        dxs.append(dx)
    close(f"gconv3x3_bwd accumulate cpg{cpg} 2x96x96", {
        "dx(use 1)": (dxs[0], refs[0][0]), "dx(use 2)": (dxs[1], refs[1][0]),
        "dweight": (bufs[0], dw0 + refs[0][1] + refs[1][1]), "dbias": (bufs[1], db0 + refs[0][2] + refs[1][2])},
        {"dx(use 1)": PIX, "dx(use 2)": PIX, "dweight": RED, "dbias": RED})


# ------------------------------------------------------------------------------------------ 5. pyramid
@pytest.mark.parametrize("shape", [(2, 64, 96, 96), (2, 64, 52, 132), (3, 5, 4, 4)], ids=["2x64x96x96", "2x64x52x132", "3x5x4x4"])
def test_pyramid_backward(AG, cuda, shape):
    """din of (x0.5, x0.25) bilinear downsampling (align_corners=False): full rows of 64, w > 64 with a partial block, one 4 x 4
    block"""
    n, c, h, w = shape
    x = R.randn64(800, n, c, h, w)
    G2, G4 = R.randn64(801, n, c, h // 2, w // 2), R.randn64(802, n, c, h // 4, w // 4)
    cx, gx = leaf(x), leaf(x, cuda)
    (ref,), (got,) = vjp(R.pyramid(cx), (G2, G4), [cx]), vjp(AG.pyramid(gx), (G2, G4), [gx])
    close(f"pyramid {'x'.join(map(str, shape))}", {"dx": (got, ref)}, PIX)


# ------------------------------------------------------------------------------------------ 6. RCAB tail, the fallback kernels
@pytest.mark.parametrize("hw", [(96, 96), (9, 7)], ids=["96x96", "9x7"])
@pytest.mark.parametrize("c,cr", [(32, 2), (64, 16)], ids=["c32_cr2", "c64_cr16"])
def test_rcab_tail_fallback_backward(AG, cuda, c, cr, hw):
    """channel counts the one-launch tail backward rejects: plane_sum -> ca_mlp_bwd -> scale_residual_bwd"""
    from eavsr_amd import ops
    assert not ops.rcab_tail_bwd_supported(c, cr)
    n = 2
    r, x, G = R.randn64(900, n, c, *hw), R.randn64(901, n, c, *hw), R.randn64(902, n, c, *hw)
    r = r + R.randn64(903, n, c, 1, 1)          # channel means away from zero: the MLP sees more than noise
    ps = [R.randn64(904, cr, c, 1, 1, scale=c ** -0.5), R.randn64(905, cr, scale=0.5),
          R.randn64(906, c, cr, 1, 1, scale=cr ** -0.5), R.randn64(907, c, scale=0.5)]
    cl = [leaf(t) for t in [r, x] + ps]
    gl = [leaf(t, cuda) for t in [r, x] + ps]
    ref = vjp(R.rcab_tail(*cl), G, cl)
    with ops.profile() as prof:
        got = vjp(AG.rcab_tail(*gl), G, gl)
    names = set(prof.summary())
    assert {"ca_mlp_bwd", "scale_residual_bwd"} <= names and "rcab_tail_bwd" not in names, names
    keys = ["dr", "dx", "dw1", "db1", "dw2", "db2"]
    close(f"rcab_tail fallback c{c} cr{cr} {hw[0]}x{hw[1]}", dict(zip(keys, zip(got, ref))),
          {k: (PIX if k in ("dr", "dx") else RED) for k in keys})


# ------------------------------------------------------------------------------------------ 7. DCNv2, sampler side, training shape
@pytest.mark.parametrize("sigma", [1.0, 6.0], ids=["sigma1", "sigma6"])
def test_dcnv2_sampler_backward_at_the_training_shape(AG, cuda, sigma):
    """csrc/dcn_bwd.hip at 2 x 64 x 96 x 96, 8 deformable groups, against float64 autograd of the oracle (not against the column
    path, which a bug shared by both would pass); sigma = 6 sends many samples out of the dx window and the image"""
    from eavsr_amd import ops
    n, c, h, w, dg = 2, 64, 96, 96, 8
    x = R.randn64(1000, n, c, h, w)
    off = R.dcn_offsets(1001, n, dg, h, w, sigma)
    mask = R.uniform64(1002, 0.0, 1.0, n, dg * 9, h, w)
    wt = R.randn64(1003, 64, c, 3, 3, scale=1.0 / 24)
    b = R.randn64(1004, 64, scale=0.1)
    G = R.randn64(1005, n, 64, h, w)
    cl = [leaf(t) for t in (x, off, mask, wt, b)]
    ref_out = R.dcnv2(*cl, dg)
    ref = vjp(ref_out, G, cl)
    gl = [leaf(t, cuda) for t in (x, off, mask, wt, b)]
    with ops.profile() as prof:
        got_out = AG.modulated_deform_conv2d(gl[0], gl[1], gl[2], gl[3], gl[4], 1, 1, 1, 1, dg)
        got = vjp(got_out, G, gl)
    names = set(prof.summary())
    assert "dcnv2_bwd" in names and "dcnv2_im2col" not in names, names
    keys = ["dx", "doffset", "dmask", "dweight", "dbias"]
    close(f"dcnv2 sampler bwd 2x64x96x96 dg8 sigma{sigma:g}", {"out": (got_out, ref_out), **dict(zip(keys, zip(got, ref)))}, RED)
