"""Bit-exact GPU tests of the 16-bit (bf16 / fp16) kernels: rounding, range edges, non-finite values.

tests/test_hip_h16.py holds these kernels to one 16-bit ulp OF THE LARGEST ELEMENT on random inputs -- a bound that truncation,
ties-away, flushed subnormals and a clamp at the largest finite value all pass.  Here the inputs come from tests/h16_exact.py:
convolutions whose fp32 accumulation is exact in every order (proved on the CPU by tests/test_h16_exact_host.py) and whose exact
results are ties, near-ties, carries, the top of the range and fp16 subnormals.  The kernel's raw output words are compared
with `V.to(dtype)` of the CPU; a NaN matches any NaN.  Every pixel that holds no target must equal the epilogue of the bias
alone, which doubles as a halo / locality check (sources sit at (0, 0), on both sides of the 8 x 32 tile seam, in the last row
and column, and in the second sample only).

No test here feeds a non-finite or large OFFSET, FLOW or COORDINATE to a sampler: non-finite values appear in feature tensors and
weights only."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import h16_exact as X

pytestmark = pytest.mark.gpu
DTS = ("bf16", "fp16")
INF, NAN = float("inf"), float("nan")

# (shape, source sets): one tile | 2 x 2 ragged tiles over two samples (all sources in the second one; two sets, because
# (7, 31) and (8, 32) are neighbours and the stamps of a launch must not overlap) | the degenerate images
MAIN = [((1, 8, 32), ((0, 0, 0), (0, 7, 31), (0, 3, 16))),
        ((2, 11, 37), ((1, 0, 0), (1, 7, 31), (1, 10, 12), (1, 4, 36))),
        ((2, 11, 37), ((1, 8, 32), (1, 10, 36), (1, 0, 20), (1, 3, 3)))]
DEGENERATE = [((1, 1, 1), ((0, 0, 0),)), ((1, 1, 40), ((0, 0, 0), (0, 0, 33), (0, 0, 39))), ((1, 33, 1), ((0, 0, 0), (0, 8, 0), (0, 32, 0)))]
THREE = [((1, 8, 32), ((0, 0, 1), (0, 7, 30), (0, 3, 16), (0, 3, 17))),
         ((2, 11, 37), ((1, 0, 1), (1, 7, 31), (1, 8, 32), (1, 10, 35), (1, 4, 1), (1, 10, 12)))]
GEOM = [("single",) + g for g in MAIN + DEGENERATE] + [("three",) + g for g in THREE]
GEOM_IDS = [f"{g[0]}-{'x'.join(map(str, g[1]))}-{i}" for i, g in enumerate(GEOM)]


@pytest.fixture(scope="module")
def ops(cuda):
    from eavsr_amd import ops as _ops
    _ops.lib()
    return _ops


@functools.lru_cache(maxsize=None)
def cases(dt, flavour, shape, sources, epilogue="none", slope=0.25, cout=64, ksize=3):
    cs = X.conv_cases(dt, shape, list(sources), flavour, epilogue, slope, cout=cout, ksize=ksize)
    assert cs
    return cs


def check(got, want, what=""):
    got, want = got.cpu(), want.cpu()
    assert X.same_bits(got, want), (what, X.mismatches(got, want))


def check_sum32(got, want, what=""):
    """an fp32 output against the exact sum, for the kernels whose BIAS IS THE MFMA's ACCUMULATOR OPERAND (conv5x5_c64_h16,
    dcnv2_il16).  Measured on gfx950: v_mfma_f32_32x32x16_bf16 with a non-zero C returns C + the three products one fp32 ulp off
    (+-inf beside fp32 max) when the sum lies in the TOP BINADE of fp32, |sum| >= 2^127 -- the rows of the bf16 table beside the
    bf16 overflow boundary; the same sums with C = 0 (the backbone kernel) and every sum below 2^127 are exact.  So: bit for bit
    below 2^127, within one fp32 ulp at and above it (DESIGN.md, 16-bit numerics)."""
    got, want = got.cpu(), want.cpu()
    top = want.abs() >= 2.0 ** 127
    assert X.same_bits(got[~top], want[~top]), (what, X.mismatches(torch.where(top, want, got), want))
    d = (X.bits_of(got[top]).long() - X.bits_of(want[top]).long()).abs()
    assert not torch.isnan(got[top]).any() and (d <= 1).all(), (what, got[top], want[top])


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(X.DT[dt])


# ---- kernels with a 16-bit output: the target table, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", ["plain", "relu", "partial", "border"])
@pytest.mark.parametrize("flavour,shape,sources", GEOM, ids=GEOM_IDS)
def test_conv3x3_c64_h16_rounds_exact_sums_to_nearest_even(ops, cuda, dt, mode, flavour, shape, sources):
    """eavsr_conv3x3_c64_h16 / _b: ties, near-ties, carries, +-0, fp16 sums of 65520 / 131072 (inf) and 65519.99 (65504), fp16
    subnormal results -- plain, through ReLU, with the channel sums and with the border pieces (the same 16-bit tensor from the
    other instantiations of the kernel; the sums against fp64 sums of the expected 16-bit values)"""
    relu = mode != "plain"
    for c in cases(dt, flavour, shape, sources, "relu" if relu else "none"):
        xh, w, b = c.nhwc16(c.x).to(cuda), c.weight.to(cuda), c.bias.to(cuda)
        want = c.want16()
        if mode in ("plain", "relu"):
            check(ops.conv3x3_c64_h16(xh, w, b, relu=relu), want, mode)
            continue
        res = ops.conv3x3_c64_h16(xh, w, b, relu=True, chan_partial=True, border=(mode == "border"))
        check(res[0], want, mode)
        w64 = want.double()
        # (sums are held to the fp64 ones where no fp32 summation order can overflow; a sample with a target beyond 65504 -- inf in
        # fp16 -- or at the top of the bf16 range is left to the non-finite test below)
        keep = w64.abs().sum((1, 2)) < 2.0 ** 120
        sums = res[1].sum(1).cpu().double()
        tol = 2e-5 * max(1.0, float(w64[torch.isfinite(w64)].abs().max())) * shape[1] * shape[2]
        assert (sums - w64.sum((1, 2)))[keep].abs().max().item() <= tol
        if mode == "border":
            h, wd = shape[1], shape[2]
            pd, pieces = res[2].data.cpu().double(), res[2]
            lines = [w64[:, 0].sum(1), w64[:, h - 1].sum(1), w64[:, :, 0].sum(1), w64[:, :, wd - 1].sum(1)]
            for bi, (line, cnt) in enumerate(zip(lines, (pieces.p_rows, pieces.p_rows, pieces.p_cols, pieces.p_cols))):
                got = pd[:, bi, :cnt].sum(1)
                k = keep & torch.isfinite(line)
                assert (got - line)[k].abs().max().item() <= tol


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("act,slope", [(None, 0.0), ("relu", 0.0), ("lrelu", 0.125), ("lrelu", 0.25)])
@pytest.mark.parametrize("flavour,shape,sources", [GEOM[0], GEOM[2], GEOM[3], GEOM[7]], ids=[GEOM_IDS[i] for i in (0, 2, 3, 7)])
def test_conv3x3_c64_h16_act_rounds_exact_sums_to_nearest_even(ops, cuda, dt, act, slope, flavour, shape, sources):
    """eavsr_conv3x3_c64_h16_act: no activation / ReLU / LeakyReLU with the exact slopes 1/8 and 1/4 (a negative target V comes from
    V / slope in front of the activation)"""
    for c in cases(dt, flavour, shape, sources, act or "none", slope or 0.25):
        out = ops.conv3x3_c64_h16_act(c.nhwc16(c.x).to(cuda), c.weight.to(cuda), c.bias.to(cuda), act=act, slope=slope)
        check(out, c.want16(), act)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("act,slope", [(None, 0.0), ("lrelu", 0.125)])
@pytest.mark.parametrize("shape,sources", [MAIN[0], MAIN[2]], ids=["1x8x32", "2x11x37"])
def test_conv3x3_c64_h16_pixel_shuffle_rounds_exact_sums_in_all_four_slices(ops, cuda, dt, act, slope, shape, sources):
    """the 64 -> 256 + PixelShuffle(2) form: four slices of the backbone kernel, each with its own weights, bias and output
    phase; the table is spread over all 256 channels, so every slice holds targets"""
    seen = set()
    for c in cases(dt, "single", shape, sources, act or "none", slope or 0.25, cout=256):
        out = ops.conv3x3_c64_h16_act(c.nhwc16(c.x).to(cuda), c.weight.to(cuda), c.bias.to(cuda), act=act, slope=slope, pixel_shuffle2=True)
        n, h, w = shape
        assert tuple(out.shape) == (n, 2 * h, 2 * w, 64)
        check(out, nhwc(F.pixel_shuffle(c.want32, 2), dt), act)
        seen |= {co % 4 for co in (c.hit >= 0).any(0).any(-1).any(-1).nonzero().flatten().tolist()}
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("flavour,shape,sources", [GEOM[0], GEOM[1], GEOM[2], GEOM[3], GEOM[5], GEOM[7]], ids=[GEOM_IDS[i] for i in (0, 1, 2, 3, 5, 7)])
def test_conv3x3_c64_h16_res_rounds_skip_plus_scale_times_conv_once(ops, cuda, dt, flavour, shape, sources):
    """eavsr_conv3x3_c64_h16_res: skip + scale[n, co] * (conv + bias) with power-of-two scales 1/4 .. 2 and a skip chosen so that
    the whole tail is exact in fp32 and lands on the table"""
    for c in cases(dt, flavour, shape, sources, "res"):
        out = ops.conv3x3_c64_h16_res(c.nhwc16(c.x).to(cuda), c.weight.to(cuda), c.bias.to(cuda), c.nhwc16(c.skip).to(cuda), c.scale.to(cuda))
        check(out, c.want16())


@pytest.mark.parametrize("dt", DTS)
def test_rcab_convs_h16_rounds_exact_sums_to_nearest_even(ops, cuda, dt):
    """the one-launch RCAB convolutions (lab build): an identity first convolution (the input is >= 0, so ReLU keeps it), the exact
    case as the second"""
    if not ops.lab_available():
        pytest.skip("ops.rcab_convs_h16 is a lab-only schedule")
    ident = torch.zeros(64, 64, 3, 3)
    ident[torch.arange(64), torch.arange(64), 1, 1] = 1.0
    for flavour, shape, sources in (GEOM[0], GEOM[2], GEOM[7]):
        for c in cases(dt, flavour, shape, sources):
            out = ops.rcab_convs_h16(c.nhwc16(c.x).to(cuda), ident.to(cuda), None, c.weight.to(cuda), c.bias.to(cuda), chan_partial=False)
            check(out, c.want16())


@pytest.mark.parametrize("dt", DTS)
def test_scale_residual_h16_rounds_exact_results_to_nearest_even(ops, cuda, dt):
    V, _ = X.targets(dt)
    for page in range(-(-V.numel() // 128)):
        r, scale, x, want, _ = X.scale_residual_case(dt, 2, 9, 13, page=page)
        out = ops.scale_residual_h16(nhwc(r, dt).to(cuda), scale.to(cuda), nhwc(x, dt).to(cuda))
        check(out, nhwc(want, dt), page)


def table_tensor(dt, n, c, h, w, shift=0):
    """the whole table, -0 and the fp16 values beside 2^-25 included, tiled over an (n, c, h, w) fp32 tensor"""
    V, _ = X.targets(dt)
    return V[(torch.arange(n * c * h * w) + shift) % V.numel()].view(n, c, h, w).clone()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(1, 64, 8, 32), (2, 64, 11, 37), (1, 24, 1, 1), (3, 8, 5, 67)])
def test_layout_converters_round_to_nearest_even(ops, cuda, dt, shape):
    """to_nhwc_h16 / to_il8_h16 on the table (with +-inf and a NaN among it); from_nhwc_h16 = exact widening + ONE fp32 add"""
    n, c, h, w = shape
    x = table_tensor(dt, n, c, h, w)
    flat = x.view(-1)
    flat[:: 97] = INF
    flat[1:: 89] = -INF
    flat[2:: 83] = NAN
    xh = ops.to_nhwc_h16(x.to(cuda), dt)
    check(xh, nhwc(x, dt))
    check(ops.to_il8_h16(x.to(cuda), dt), x.view(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().to(X.DT[dt]))
    g = torch.Generator().manual_seed(7)
    res = torch.randn(n, c, h, w, generator=g) * table_tensor(dt, n, c, h, w, shift=5).abs().clamp(2.0 ** -20, 2.0 ** 20)
    check(ops.from_nhwc_h16(xh, residual=res.to(cuda)), x.to(X.DT[dt]).float() + res)
    check(ops.from_nhwc_h16(xh), x.to(X.DT[dt]).float())


@pytest.mark.parametrize("dt", DTS)
def test_from_nhwc_h16_widens_every_16_bit_pattern_exactly(ops, cuda, dt):
    """all 65536 words -- subnormals, infinities and NaNs included -- as one (1, 32, 32, 64) tensor"""
    words = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(1, 32, 32, 64)
    xh = words.view(X.DT[dt])
    want = xh.float().permute(0, 3, 1, 2).contiguous()
    check(ops.from_nhwc_h16(xh.to(cuda)), want)
    res = torch.full_like(want, 0.75)
    check(ops.from_nhwc_h16(xh.to(cuda), residual=res.to(cuda)), want + res)


@pytest.mark.parametrize("dt", DTS)
def test_flow_warp_pair_16bit_output_rounds_to_nearest_even(ops, cuda, dt):
    """the IL8 16-bit output of the paired warp with INTEGER flows (small, finite): the blend is 1 * v + 0 + 0 + 0, exact, so the
    output is the rounded table (-0 as +0: it is added to the zero products).  h - 1 and w - 1 are powers of two: the kernel
    normalises and un-normalises its coordinates as the reference's grid_sample call does, and only then is that round trip exact
    (at w = 37 an integer coordinate comes back one ulp off, and the blend mixes in a neighbour at weight 1e-7)."""
    n, c, h, w = 2, 64, 9, 65
    xb = table_tensor(dt, n, c, h, w) + 0.0
    xa = table_tensor(dt, n, c, h, w, shift=11) + 0.0
    fy = (torch.arange(h).view(1, h, 1) % 3 - 1).expand(n, h, w)
    fx = (torch.arange(w).view(1, 1, w) % 5 - 2).expand(n, h, w)
    flow = torch.stack((fx, fy), 1).float().contiguous()
    ys, xs = torch.arange(h).view(1, h, 1) + fy, torch.arange(w).view(1, 1, w) + fx
    ok = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    idx = (ys.clamp(0, h - 1) * w + xs.clamp(0, w - 1)).view(n, 1, h * w).expand(n, c, h * w)
    warp = lambda t: torch.where(ok.view(n, 1, h, w), t.view(n, c, h * w).gather(2, idx).view(n, c, h, w), torch.zeros(()))
    a32, b16 = ops.flow_warp_pair(xa.to(cuda), xb.to(cuda), flow.to(cuda), b_il8=dt)
    # inside the frame: bit for bit.  A sample outside the frame is zero of EITHER sign: the (fp32) blend multiplies its clamped
    # corners by a zero weight, so four negative corners give -0 where grid_sample gives +0 -- a property of the fp32 warp that
    # the 16-bit output inherits, measured here and not this test's subject (DESIGN.md, 16-bit numerics)
    okc = ok.view(n, 1, h, w).expand(n, c, h, w)
    il = lambda t: t.view(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()
    a32, b16 = a32.cpu(), b16.cpu()
    check(a32[okc], warp(xa)[okc])
    check(b16[il(okc)], il(warp(xb)).to(X.DT[dt])[il(okc)])
    assert (a32[~okc] == 0).all() and (b16[~il(okc)].float() == 0).all() and (~okc).any()


# ---- fp32 in, operands rounded once (conv2d under set_conv3_h16) ---------------------------------------------------------------
def overflowing(dt):
    V, _ = X.targets(dt)
    return torch.isinf(V.to(X.DT[dt]).float())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("k,cin,cout,shape", [(3, 64, 64, (2, 11, 36)), (7, 32, 16, (2, 11, 37)), (3, 64, 64, (1, 8, 32)), (7, 32, 16, (1, 9, 12))])
def test_conv2d_h16_routes_round_each_operand_once(ops, cuda, dt, k, cin, cout, shape):
    """the h16g 3x3 and the h16x1 7x7 routes: the table in x under one-hot weights of 1.0, and in the weights under a one-hot input
    -- the fp32 output is V.to(dtype).float() (a value that rounds to inf makes 0 * inf = NaN where a zero weight / input meets
    it: the fp64 convolution of the rounded operands says where)"""
    n, h, w = shape
    V, _ = X.targets(dt)
    fin = V[~overflowing(dt)]
    over = V[overflowing(dt)] if h * w >= 200 else V[:0]      # (in a 9 x 12 image their 7 x 7 NaN footprints would cover everything)
    name = f"conv{k}x{k}_{cin}to{cout}_h16" + ("g" if k == 3 else "x1")
    # (a) the table in x
    x = fin[torch.arange(n * cin * h * w) % fin.numel()].view(n, cin, h, w).clone()
    spots = [(n - 1, min(7, h - 1), min(31, w - 1)), (n - 1, 0, 0), (0, h - 1, w // 2)]
    for j, v in enumerate(over.tolist()):          # a value that overflows the type: alone in its pixel
        a_, y_, x_ = spots[j % len(spots)]
        x[a_, :, y_, x_] = 0.0
        x[a_, (5 * j) % cin, y_, x_] = v
        spots[j % len(spots)] = (a_, y_, (x_ + 4) % w)
    wt = torch.zeros(cout, cin, k, k)
    wt[torch.arange(cout), torch.arange(cout) * (cin // cout if cin >= cout else 1) % cin, k // 2, k // 2] = 1.0
    ref = F.conv2d(x.to(X.DT[dt]).double(), wt.double(), None, 1, k // 2).float()
    sel = x.to(X.DT[dt]).float()[:, torch.arange(cout) * (cin // cout if cin >= cout else 1) % cin] + 0.0
    okm = ~torch.isnan(ref)
    assert torch.equal(ref[okm], sel[okm]) and okm.float().mean() > 0.5       # the reference IS the rounded table
    ops.set_conv3_h16(dt)
    try:
        with torch.no_grad(), ops.profile() as prof:
            got = ops.conv2d(x.to(cuda), wt.to(cuda), None)
        assert name in prof.summary(), list(prof.summary())
        check(got, ref, "table in x")
        # (b) the table in the weights: w[:, ci0] holds it, the input is 1.0 in channel ci0 of one pixel per sample
        ci0 = cin - 3
        wt2 = torch.zeros(cout, cin, k, k)
        tab = torch.cat([fin, over])
        wt2[:, ci0] = tab[torch.arange(cout * k * k) % tab.numel()].view(cout, k, k)
        x2 = torch.zeros(n, cin, h, w)
        x2[0, ci0, min(7, h - 1), min(31, w - 1)] = 1.0
        x2[n - 1, ci0, h // 2, 3] = 1.0
        ref2 = F.conv2d(x2.double(), wt2.to(X.DT[dt]).double(), None, 1, k // 2).float()
        with torch.no_grad(), ops.profile() as prof:
            got2 = ops.conv2d(x2.to(cuda), wt2.to(cuda), None)
        assert name in prof.summary(), list(prof.summary())
        check(got2, ref2, "table in the weights")
    finally:
        ops.set_conv3_h16(None)


# ---- 16-bit in, fp32 out: operands arrive unflushed and unswapped, the sum is exact --------------------------------------------
SUBNORMALS = [1, 2, 3, 5, 512, 1023]      # multiples of the fp16 subnormal step 2^-24


def subnormal_case(n, h, w, cout, ksize):
    """fp16 SUBNORMAL inputs times a normal weight (2^10): x holds m * 2^-24 in channel 5 of a few pixels, the centre tap of
    every output channel holds 2^10 * (1 + co % 2) for that channel: out = 2^-14 * m * (1 + co % 2), exact"""
    x = torch.zeros(n, 64, h, w, dtype=torch.float64)
    for j, m in enumerate(SUBNORMALS):
        x[j % n, 5, (3 * j) % h, (7 * j) % w] = m * 2.0 ** -24
    wt = torch.zeros(cout, 64, ksize, ksize, dtype=torch.float64)
    wt[:, 5, ksize // 2, ksize // 2] = 1024.0 * (1 + torch.arange(cout) % 2)
    return x.float(), wt.float(), F.conv2d(x, wt, None, 1, ksize // 2).float()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("shape,sources", MAIN + DEGENERATE[:1], ids=[str(i) for i in range(4)])
def test_conv3x3_c64to3_h16_sums_exactly(ops, cuda, dt, res, shape, sources):
    """conv_last (v_dot2 on 16-bit pairs, the bias as the accumulator's first value): the exact sum in fp32, then ONE fp32 add of
    the skip image"""
    g = torch.Generator().manual_seed(3)
    for c in cases(dt, "single", shape, sources, cout=3):
        r = torch.randn(c.want32.shape, generator=g) * c.want32.abs().clamp(2.0 ** -20, 2.0 ** 20) if res else None
        got = ops.conv3x3_c64to3_h16(c.nhwc16(c.x).to(cuda), c.weight.to(cuda), c.bias.to(cuda), residual=None if r is None else r.to(cuda))
        check(got, c.want32 + r if res else c.want32)
    if dt == "fp16":
        x, wt, want = subnormal_case(*shape, 3, 3)
        check(ops.conv3x3_c64to3_h16(nhwc(x, dt).to(cuda), wt.to(cuda), None), want, "subnormal inputs")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape,sources", [((1, 8, 32), ((0, 0, 0), (0, 7, 31), (0, 3, 16))), ((2, 11, 37), ((1, 0, 0), (1, 7, 31), (1, 10, 12), (1, 4, 36))),
                                           ((2, 11, 37), ((1, 8, 32), (1, 10, 8), (1, 0, 20), (1, 3, 3)))], ids=["0", "1", "2"])
def test_conv5x5_c64_h16_sums_exactly(ops, cuda, dt, shape, sources):
    """the predictor's 5x5 heads (three heads as one 72-channel launch): fp32 output = the exact sum"""
    for c in cases(dt, "single", shape, sources, cout=72, ksize=5):
        ws, bs = list(c.weight.split((32, 16, 24))), list(c.bias.split((32, 16, 24)))
        got = ops.conv5x5_c64_h16(c.nhwc16(c.x).to(cuda), [w_.to(cuda) for w_ in ws], [b_.to(cuda) for b_ in bs])
        check_sum32(got, c.want32)
    if dt == "fp16":
        x, wt, want = subnormal_case(*shape, 40, 5)
        check(ops.conv5x5_c64_h16(nhwc(x, dt).to(cuda), wt.to(cuda), None), want, "subnormal inputs")


def il8(x, dt):
    n, c, h, w = x.shape
    return x.view(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().to(X.DT[dt])


def dcn_zero_offsets(n, h, w, D, heads, cuda):
    """explicit: zero offsets and unit masks; heads: identity transforms, zero translations, mask logits of 40 (sigmoid = 1.0)"""
    if not heads:
        return torch.zeros(n, 18 * D, h, w, device=cuda), torch.ones(n, 9 * D, h, w, device=cuda)
    hd = torch.zeros(n, 15 * D, h, w)
    hd[:, 0:4 * D:4] = 1.0
    hd[:, 3:4 * D:4] = 1.0
    hd[:, 6 * D:] = 40.0
    return hd.to(cuda), None


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("shape,sources", MAIN + DEGENERATE, ids=[str(i) for i in range(6)])
def test_dcnv2_il16_with_zero_offsets_sums_exactly(ops, cuda, dt, heads, shape, sources):
    """DCNv2 in 16 bits with zero offsets and unit masks is the plain convolution: every blended sample is 1 * v + 0 + 0 + 0 and
    its rounding to 16 bits the identity, so the fp32 output is the exact sum"""
    n, h, w = shape
    off, mask = dcn_zero_offsets(n, h, w, 8, heads, cuda)
    for c in cases(dt, "single", shape, sources):
        got = ops.dcnv2_il16(il8(c.x, dt).to(cuda), off, mask, c.weight.to(cuda), c.bias.to(cuda), 8, heads=heads)
        check_sum32(got, c.want32)
    if dt == "fp16":
        x, wt, want = subnormal_case(n, h, w, 64, 3)
        check(ops.dcnv2_il16(il8(x, dt).to(cuda), off, mask, wt.to(cuda), None, 8, heads=heads), want, "subnormal inputs")


@pytest.mark.parametrize("shape,sources", MAIN[1:2], ids=["2x11x37"])
def test_conv3x3_c64_h16_takes_fp16_subnormal_inputs(ops, cuda, shape, sources):
    """the matrix pipe with fp16 subnormal B operands: m * 2^-24 times 2^10 (or 2^11) is a normal fp16 number, exactly"""
    x, wt, want = subnormal_case(*shape, 64, 3)
    check(ops.conv3x3_c64_h16(nhwc(x, "fp16").to(cuda), wt.to(cuda), None), nhwc(want, "fp16"))


# ---- non-finite values and the top of the range ---------------------------------------------------------------------------------
FREE = (15, 31, 47)      # input channels no scale group of the exact cases uses
_finite_cases = {}


def nonfinite_case(dt, plan):
    """an exact case on (2, 11, 37) with non-finite inputs added: `plan` = [(value, sample, y, x)], value j in free input channel
    FREE[j] whose weights are 1/8 in every tap of every output channel (all positive)"""
    if dt not in _finite_cases:      # (the rows of the table that stay finite in the type: "every other pixel is finite")
        V, labels = X.targets(dt)
        fin = torch.tensor([l_ != "top" for l_ in labels])      # (and whose fp32 sums cannot overflow)
        tab = (V[fin], [l_ for l_, f_ in zip(labels, fin.tolist()) if f_])
        _finite_cases[dt] = X.conv_cases(dt, (2, 11, 37), [(1, 0, 0), (1, 4, 36), (0, 10, 20)], "single", table=tab)[0]
    c = _finite_cases[dt]
    x, wt = c.x.clone(), c.weight.clone()
    for j, (v, a_, y_, x_) in enumerate(plan):
        x[a_, FREE[j], y_, x_] = v
        wt[:, FREE[j]] = 0.125
    pre = F.conv2d(x.double(), wt.double(), c.bias.double(), 1, 1)
    return c, x, wt, pre


PLANS = {"infs": [(INF, 0, 7, 31), (-INF, 1, 8, 32)], "nan": [(NAN, 1, 7, 32)], "all": [(INF, 0, 8, 31), (-INF, 1, 7, 32), (NAN, 1, 3, 12)]}


def hood(n, h, w, plan, kind):
    m = torch.zeros(n, h, w, dtype=torch.bool)
    for (v, a_, y_, x_) in plan:
        if kind(v):
            m[a_, max(y_ - 1, 0):y_ + 2, max(x_ - 1, 0):x_ + 2] = True
    return m


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_conv3x3_c64_h16_family_with_inf_and_nan_inputs(ops, cuda, dt, plan):
    """+inf / -inf / NaN in one channel of one pixel on a tile seam, all-positive weights for that channel: the 3 x 3 neighbourhood
    is +-inf / NaN in every output channel and EVERY OTHER PIXEL IS BIT-EXACT AND FINITE; through ReLU a NaN stays a NaN and -inf
    becomes +0, as torch.relu gives (fmaxf(NaN, 0) = 0: the epilogue's ReLU is a select); the channel sums and border pieces are
    inf / NaN exactly where the fp64 sums are.  Reference: F.conv2d in fp64 on the same 16-bit operands, the exact epilogue,
    .to(dtype)."""
    c, x, wt, pre = nonfinite_case(dt, PLANS[plan])
    n, h, w = 2, 11, 37
    xh, gw, gb = nhwc(x, dt).to(cuda), wt.to(cuda), c.bias.to(cuda)
    isinf_, isnan_ = hood(n, h, w, PLANS[plan], lambda v: v in (INF, -INF)), hood(n, h, w, PLANS[plan], lambda v: v != v)
    want = nhwc(pre.float(), dt)
    assert torch.equal(torch.isinf(want.float()).all(-1), isinf_) and torch.equal(torch.isnan(want.float()).all(-1), isnan_)
    assert torch.isfinite(want.float()[~(isinf_ | isnan_)]).all()
    check(ops.conv3x3_c64_h16(xh, gw, gb), want, "plain")
    check(ops.conv3x3_c64_h16_act(xh, gw, gb, act=None), want, "act none")
    wr = nhwc(torch.relu(pre).float(), dt)
    assert torch.isnan(wr.float()[isnan_]).all() and not torch.signbit(wr.float()[wr.float() == 0]).any()
    check(ops.conv3x3_c64_h16(xh, gw, gb, relu=True), wr, "relu")
    check(ops.conv3x3_c64_h16_act(xh, gw, gb, act="relu"), wr, "act relu")
    check(ops.conv3x3_c64_h16_act(xh, gw, gb, act="lrelu", slope=0.25), nhwc(F.leaky_relu(pre, 0.25).float(), dt), "act lrelu")
    scale = torch.tensor([[X._scale_of(a_, co) for co in range(64)] for a_ in range(n)])
    skip = torch.full((n, 64, h, w), 0.5)
    wres = nhwc((skip.double() + scale.double().view(n, 64, 1, 1) * pre).float(), dt)
    check(ops.conv3x3_c64_h16_res(xh, gw, gb, nhwc(skip, dt).to(cuda), scale.to(cuda)), wres, "res")
    for relu, wv in ((False, want), (True, wr)):
        out, part, pieces = ops.conv3x3_c64_h16(xh, gw, gb, relu=relu, chan_partial=True, border=True)
        check(out, wv, "border")
        w64 = wv.double()
        lines = [w64.sum((1, 2)), w64[:, 0].sum(1), w64[:, h - 1].sum(1), w64[:, :, 0].sum(1), w64[:, :, w - 1].sum(1)]
        pd = pieces.data.cpu().double()
        gots = [part.sum(1).cpu().double()] + [pd[:, bi, :cnt].sum(1) for bi, cnt in enumerate((pieces.p_rows, pieces.p_rows, pieces.p_cols, pieces.p_cols))]
        for got, line in zip(gots, lines):
            k = torch.isfinite(line)
            assert torch.equal(torch.isnan(got), torch.isnan(line)) and torch.equal(got[torch.isinf(line)], line[torch.isinf(line)])
            assert not k.any() or (got - line)[k].abs().max().item() <= 2e-5 * h * w * max(1.0, float(w64[torch.isfinite(w64)].abs().max()))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_dcnv2_il16_with_inf_and_nan_inputs(ops, cuda, dt, heads, plan):
    """the same non-finite feature values through the 16-bit DCNv2 with ZERO offsets and unit masks (finite, small sampling
    coordinates only) against F.conv2d in fp64 on the same 16-bit operands.

    A bilinear sample is w1 v1 + w2 v2 + w3 v3 + w4 v4 over its four corners, and at an integer position three of the weights are
    0: as a plain product a sample NEXT to the non-finite pixel would be 0 * inf = NaN (448 / 1920 / 2368 of these 52096 values were
    NaN where the convolution is finite or inf before the kernel read zero-weight corners from a zero unit instead of the window;
    csrc/dcnv2_il16.hip, `s_zero`).  A corner at weight 0 contributes nothing, whatever it holds."""
    c, x, wt, pre = nonfinite_case(dt, PLANS[plan])
    n, h, w = 2, 11, 37
    off, mask = dcn_zero_offsets(n, h, w, 8, heads, cuda)
    got = ops.dcnv2_il16(il8(x, dt).to(cuda), off, mask, wt.to(cuda), c.bias.to(cuda), 8, heads=heads)
    check(got, pre.float())


@pytest.mark.parametrize("dt", DTS)
def test_ca_scale_pre_h16_with_inf_and_nan_sums(ops, cuda, dt):
    """the attention before the second convolution on a t that holds +inf (sample 0) and a NaN (sample 1) away from the image
    border, with an all-positive second convolution: every channel mean of sample 0 is +inf, so a hidden unit is +inf (positive
    weights), 0 (negative weights: ReLU(-inf)) -- and the attention is sigmoid(+inf) = 1, sigmoid(-inf) = 0 or, where +inf and
    -inf meet, NaN; sample 1 is NaN throughout (CALayer's ReLU keeps a NaN; fmaxf would have made the hidden unit 0 and the
    attention finite).  Against the fp64 restatement of the block (as tests/test_hip_ops.py states it for the fp32 path)."""
    c, x, wt, pre = nonfinite_case(dt, [(INF, 0, 7, 31), (NAN, 1, 5, 12)])
    n, h, w = 2, 11, 37
    t, tpart, pieces = ops.conv3x3_c64_h16(nhwc(x, dt).to(cuda), wt.to(cuda), c.bias.to(cuda), relu=True, chan_partial=True, border=True)
    check(t, nhwc(torch.relu(pre).float(), dt))
    w2 = (2.0 ** -(4 + torch.arange(64 * 64 * 9) % 3)).view(64, 64, 3, 3).float()
    b2 = torch.full((64,), 0.25)
    a_w = torch.stack([torch.full((64,), 0.5), torch.full((64,), -0.25), torch.full((64,), 0.125), torch.full((64,), -1.0)])
    a_b = torch.tensor([0.1, -0.2, 0.3, 0.4])
    c_w = torch.tensor([[1.0, 0.5, 2.0, 0.25], [-1.0, 0.5, -2.0, 0.25], [1.0, 0.5, -2.0, 0.25], [0.5, 1.0, 0.5, 1.0]]).repeat(16, 1)
    c_b = torch.linspace(-1, 1, 64)
    t64 = t.cpu().float().double().permute(0, 3, 1, 2)
    r64 = F.conv2d(t64, w2.to(X.DT[dt]).double(), b2.double(), 1, 1)
    m64 = r64.mean((2, 3))
    hid = torch.relu((m64[:, None, :] * a_w.double()[None]).sum(-1) + a_b.double())
    s64 = torch.sigmoid((hid[:, None, :] * c_w.double()[None]).sum(-1) + c_b.double())
    assert torch.isinf(m64[0]).all() and torch.isnan(m64[1]).all()
    assert set(s64[0].tolist()[:2]) == {1.0, 0.0} and torch.isnan(s64[0, 2]) and torch.isnan(s64[1]).all()
    g = lambda v: v.to(cuda)
    for border in (None, pieces):
        s = ops.ca_scale_pre_h16(t, tpart, g(w2), g(b2), g(a_w), g(a_b), g(c_w), g(c_b), border=border).cpu()
        assert torch.equal(torch.isnan(s), torch.isnan(s64)), (s, s64)
        sat = (s64 == 0) | (s64 == 1)
        assert sat.sum() == 48 and torch.equal(s[sat].double(), s64[sat])
    # a NaN among the second convolution's weights -- payload in the low mantissa bits, where a rounding add's carry would turn it
    # into an infinity -- reaches every attention value as a NaN (csrc/ca.hip rounds those weights to the 16-bit type itself)
    gen = torch.Generator().manual_seed(11)
    xf = torch.randn(n, 64, h, w, generator=gen)
    w1 = torch.randn(64, 64, 3, 3, generator=gen) / 24.0
    tf, tfp = ops.conv3x3_c64_h16(nhwc(xf, dt).to(cuda), g(w1), None, relu=True, chan_partial=True)
    assert torch.isfinite(tf.float()).all()
    w2n = w2.clone()
    w2n.view(-1)[12345] = X.f32_from_bits([0x7F800001])[0]
    assert torch.isnan(w2n.view(-1)[12345])
    assert torch.isfinite(ops.ca_scale_pre_h16(tf, tfp, g(w2), g(b2), g(a_w), g(a_b), g(c_w), g(c_b))).all()
    assert torch.isnan(ops.ca_scale_pre_h16(tf, tfp, g(w2n), g(b2), g(a_w), g(a_b), g(c_w), g(c_b))).all()
