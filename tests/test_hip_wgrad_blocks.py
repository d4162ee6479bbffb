"""The weight-gradient kernels of csrc/conv_wgrad.hip at every 64 x 64 channel block and on both sides of their slab caps.

ops.conv_wgrad / ops.conv_wgrad_multi walk a weight gradient in 64 x 64 channel blocks (co0, ci0, ci_dst0; co_valid / ci_valid
below 64 at the ragged end) and each kernel walks its pixel tiles with a grid-stride loop once there are more tiles than slabs.
Every case here is compared with torch.nn.grad.conv2d_weight of the concatenated sources in float64 on the CPU, summed over the
uses, and the bias gradient with dy.double().sum((0, 2, 3)): the whole (cout, cin, k, k) tensor and the whole (cout,) bias, on top
of a sentinel (accumulate=False) or of a known random tensor (accumulate=True).

Routes, as csrc/conv_wgrad.hip selects them: 3x3 with w % 4 == 0 and 16-byte aligned tensors runs the bf16x6 kernel
(conv_wgrad3_x6_kernel<3>, 4 x 32-pixel tiles, at most 128 slabs and never more than eavsr_conv_wgrad_blocks); any other 3x3 the
fp32-MFMA kernel (conv_wgrad3_kernel, 8 x 32 tiles, at most 256 slabs); 1x1 and 5x5 conv_wgrad_kernel<1> / <5> (8 x 32 and 4 x 32
tiles); 1x1 with a source wider than 64 channels through ops.conv_wgrad the span entry (every 64-channel block of a source in one
launch); precision="bf16" conv_wgrad3_x6_kernel<1>.  EAVSR_WGRAD3=fp32 is read once per process: the fp32 3x3 kernel is reached
here through w % 4 != 0 and through 4-byte aligned tensors, not by toggling it."""
import pytest
import torch

from tests import helpers as H
from tests import train_bf16_refs as R
from tests.golden import cases
from tests.test_hip_train_bf16 import WGRAD_BOUND

pytestmark = pytest.mark.gpu

TOL = 2e-5              # max |got - want| <= TOL * max(1, max |want|): the bound of the existing weight-gradient tests
SENTINEL = -777.0       # what an element the kernels never wrote still holds
X6_MAX_SLABS = 128      # conv_wgrad3_x6_kernel: two 4-wave workgroups per CU
MAX_SLABS = 256         # eavsr_conv_wgrad_blocks

# (sources -> cout) of the model's own 3x3 convolutions, and blocks that are ragged on both sides
CHANNELS = [((64,), 3), ((64,), 6), ((18,), 2), ((64,), 256), ((3,), 64), ((256,), 64), ((32, 16, 72), 120), ((3, 64), 72),
            ((136,), 8)]
SMALL = [(2, 12, 40), (1, 7, 36)]       # w % 4 == 0: several tiles of every kernel, the last one cut in both directions
ENTRIES = ("single", "single_acc", "multi1", "multiN", "multiN_acc")


def _ids(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return str(v)


def _cdiv(a, b):
    return -(-a // b)


def _need_x6(ops):
    if ops.lib().eavsr_wgrad3_mode() != 1:
        pytest.skip("EAVSR_WGRAD3=fp32: the bf16x6 3x3 weight-gradient kernel is switched off in this process")


def _scale(c, c0=0):
    """a scale of its own for every channel: a block that lands in another co or ci row is off by 1/64 of its value at least"""
    return (1.0 + (torch.arange(c, dtype=torch.float32) + c0) / 64.0).view(1, c, 1, 1)


def _inputs(chans, cout, n, h, w, nseg, scaled):
    dys, xs = [], []
    for s in range(nseg):
        dy = cases.randn(3000 + s, n, cout, h, w)
        ss, c0 = [], 0
        for j, c in enumerate(chans):
            x = cases.randn(4000 + 10 * s + j, n, c, h, w)
            ss.append(x * _scale(c, c0) if scaled else x)
            c0 += c
        dys.append(dy * _scale(cout) if scaled else dy)
        xs.append(ss)
    return dys, xs


def _wgrad64(k, dy, x):
    cout, cin = dy.shape[1], x.shape[1]
    if dy.shape[0] == 0:
        return torch.zeros(cout, cin, k, k, dtype=torch.float64)
    return torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), dy.double(), padding=k // 2)


def _dev(t, cuda, misaligned=False):
    """t on the device: 16-byte aligned, or a contiguous view that starts one float into a flat buffer"""
    if not misaligned:
        d = t.to(cuda)
        assert d.data_ptr() % 16 == 0
        return d
    flat = torch.empty(t.numel() + 1, device=cuda)
    d = flat[1:].view(t.shape)
    d.copy_(t)
    assert d.is_contiguous() and d.data_ptr() % 16 != 0 and d.data_ptr() % 4 == 0
    return d


def _exercise(cuda, k, chans, cout, shape, nseg=3, scaled=True, mis=None, precision="fp32", entries=ENTRIES):
    """Both entry points on the same inputs: ops.conv_wgrad on the first use (on a sentinel, then on top of a pre-filled tensor),
    ops.conv_wgrad_multi with its bias gradient on one use and on all `nseg` (the same two ways).  Every launch runs twice and
    must repeat bit for bit (slabs added in a fixed order, no atomics).  mis="all": every tensor 4-byte aligned; "one": only the
    last source of the last use.  precision="bf16": the reference is the float64 gradient of the inputs rounded to bf16 (nearest
    even) and the bound WGRAD_BOUND * max S, S the same sum over |dy| |x|; the bias gradient is that of the unrounded dy."""
    from eavsr_amd import ops
    n, h, w = shape
    cin = sum(chans)
    dys, xs = _inputs(chans, cout, n, h, w, nseg, scaled)
    if precision == "bf16":
        zero = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
        refs = [R.wgrad3x3_ref([R.bf16_rne(d)], [R.bf16_rne(torch.cat(ss, 1))]) if n else (zero, zero) for d, ss in zip(dys, xs)]
        wants, sabs = [g for g, _ in refs], [s_ for _, s_ in refs]
    else:
        wants = [_wgrad64(k, d, torch.cat(ss, 1)) for d, ss in zip(dys, xs)]
    want_bs = [d.double().sum((0, 2, 3)) for d in dys]
    base_w, base_b = cases.randn(5000, cout, cin, k, k, scale=3.0), cases.randn(5001, cout, scale=3.0)
    for entry in entries:
        used = nseg if entry.startswith("multiN") else 1
        acc = entry.endswith("_acc")
        single = entry.startswith("single")
        gd = [_dev(dys[s], cuda, mis == "all") for s in range(used)]
        gx = [[_dev(x, cuda, mis == "all" or (mis == "one" and s == used - 1 and j == len(chans) - 1)) for j, x in enumerate(xs[s])]
              for s in range(used)]
        if precision == "bf16":
            assert ops.wgrad_bf16_takes(gd, gx, k), (entry, shape)

        def run():
            out = (base_w if acc else torch.full((cout, cin, k, k), SENTINEL)).to(cuda, copy=True)
            if single:
                got = ops.conv_wgrad(gd[0], gx[0], k, out=out, accumulate=acc, precision=precision)
                assert got.data_ptr() == out.data_ptr()
                return out.cpu(), None
            db = (base_b if acc else torch.full((cout,), SENTINEL)).to(cuda, copy=True)
            ops.conv_wgrad_multi(gd, gx, k, out=out, accumulate=acc, bias_out=db, precision=precision)
            return out.cpu(), db.cpu()

        got, got_b = run()
        again, again_b = run()
        assert torch.equal(got, again), (entry, "two runs differ")
        want = sum(wants[:used]) + (base_w.double() if acc else 0.0)
        if precision == "bf16":
            bound = WGRAD_BOUND * sum(sabs[:used]).max().item()
        else:
            bound = TOL * max(1.0, want.abs().max().item())
        err = H.maxabs(got, want)
        print(f"k={k} {chans}->{cout} {shape} x{used} {entry} {precision} mis={mis}: dW err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (entry, err, bound)
        if got_b is not None:
            assert torch.equal(got_b, again_b), (entry, "two runs differ (bias)")
            want_b = sum(want_bs[:used]) + (base_b.double() if acc else 0.0)
            bound_b = 1e-5 * max(1.0, want_b.abs().max().item()) + 1e-4
            err_b = H.maxabs(got_b, want_b)
            print(f"    bias err {err_b:.3e} bound {bound_b:.3e}")
            assert err_b <= bound_b, (entry, "bias", err_b, bound_b)


# ------------------------------------------------------------------------------------------- 1. channel blocks, bf16x6 3x3
@pytest.mark.parametrize("shape", SMALL, ids=_ids)
@pytest.mark.parametrize("chans,cout", CHANNELS, ids=_ids)
def test_channel_blocks_on_the_bf16x6_3x3_kernel(cuda, chans, cout, shape):
    """w % 4 == 0 and aligned tensors: co0 and ci0 beyond the first block, ragged co_valid (2, 3, 6, 8, 56) and ci_valid (3, 8, 16,
    18), ci_dst0 behind a source that is no multiple of 64, quadrants without a valid channel"""
    from eavsr_amd import ops
    _need_x6(ops)
    _exercise(cuda, 3, chans, cout, shape)


# ------------------------------------------------------------------------------------------- 2. the same on the fp32 kernels
@pytest.mark.parametrize("chans,cout", CHANNELS, ids=_ids)
def test_channel_blocks_on_the_fp32_3x3_kernel(cuda, chans, cout):
    """w % 4 != 0: conv_wgrad3_kernel whatever the mode"""
    _exercise(cuda, 3, chans, cout, (2, 12, 38))


@pytest.mark.parametrize("mis", ["all", "one"])
@pytest.mark.parametrize("chans,cout", CHANNELS, ids=_ids)
def test_channel_blocks_with_four_byte_aligned_tensors(cuda, chans, cout, mis):
    """w % 4 == 0 but a tensor that float4 loads cannot read: the launch falls back to the fp32 kernel.  "all": dy and every
    source start one float into their buffers; "one": only the last source of the last use does, so that with several sources
    the aligned ones stay on the bf16x6 kernel and one gradient is assembled from both"""
    _exercise(cuda, 3, chans, cout, (2, 12, 40), mis=mis)


@pytest.mark.parametrize("shape", SMALL, ids=_ids)
@pytest.mark.parametrize("k,chans,cout", [(5, (64,), 120), (5, (40,), 8), (1, (64, 64, 64), 64), (1, (24,), 72)], ids=_ids)
def test_channel_blocks_on_the_5x5_and_1x1_kernels(cuda, k, chans, cout, shape):
    _exercise(cuda, k, chans, cout, shape)


# ------------------------------------------------------------------------------------------- 3. the span path
@pytest.mark.parametrize("shape", SMALL, ids=_ids)
@pytest.mark.parametrize("chans,cout", [((576,), 64), ((136,), 72), ((72, 8), 3)], ids=_ids)
def test_span_of_source_blocks_in_one_launch(cuda, chans, cout, shape):
    """k == 1 and a source wider than 64 channels: ops.conv_wgrad launches every 64-channel block of a source at once
    (blockIdx.y; DCNv2's 576-channel column tensor), with cin_src % 64 != 0, cout > 64 and a narrow source behind a wide one;
    ops.conv_wgrad_multi walks the same blocks one launch each"""
    _exercise(cuda, 1, chans, cout, shape)


# ------------------------------------------------------------------------------------------- 4. tiles against slabs
# (k, sources, cout, n, nseg, h, w, tiles, slabs): the last tile is cut in both directions in every case
FP32_TILES = [(3, (12,), 10, 5, 3, 131, 30, 255, 255), (3, (12,), 10, 2, 2, 61, 226, 256, 256), (3, (12,), 10, 1, 1, 5, 8194, 257, 256),
              (3, (12,), 10, 3, 3, 19, 578, 513, 256), (1, (12,), 10, 3, 1, 66, 290, 270, 256), (1, (72,), 10, 3, 1, 66, 290, 270, 256),
              (5, (12,), 10, 2, 1, 50, 290, 260, 256)]


@pytest.mark.parametrize("k,chans,cout,n,nseg,h,w,tiles,slabs", FP32_TILES,
                         ids=[f"k{c[0]}-{c[1][0]}ch-{c[7]}tiles" for c in FP32_TILES])
def test_fp32_kernels_with_more_tiles_than_slabs(cuda, k, chans, cout, n, nseg, h, w, tiles, slabs):
    """The grid-stride loops of conv_wgrad3_kernel (w % 4 != 0), conv_wgrad_kernel<1> (also as the span launch: 72 channels) and
    <5>: one tile per workgroup (255, 256), one workgroup with two (257), one with three among twos (513), 270 and 260 tiles.
    The sums are up to 99 K pixels long; the bound stays TOL."""
    from eavsr_amd import ops
    th = 8 if k <= 3 else 4
    assert n * nseg * _cdiv(h, th) * _cdiv(w, 32) == tiles and w % 4 != 0
    assert ops.lib().eavsr_conv_wgrad_blocks(n * nseg, h, w, k) == min(tiles, MAX_SLABS) == slabs
    _exercise(cuda, k, chans, cout, (n, h, w), nseg=nseg, scaled=False, entries=("single", "multi1") if nseg == 1 else ("multiN",))


# (n, nseg, h, w, tiles, slabs)
X6_TILES = [(1, 1, 3, 4036, 127, 127), (2, 2, 3, 996, 128, 128), (1, 3, 2, 1348, 129, 128), (2, 2, 6, 996, 256, 128),
            (1, 1, 3, 8196, 257, 128), (1, 1, 506, 28, 127, 64), (1, 1, 8, 32, 2, 1)]


@pytest.mark.parametrize("n,nseg,h,w,tiles,slabs", X6_TILES, ids=[f"{c[4]}tiles-{c[5]}slabs" for c in X6_TILES])
def test_bf16x6_kernel_next_to_its_slab_caps(cuda, n, nseg, h, w, tiles, slabs):
    """conv_wgrad3_x6_kernel<3>: slabs = min(tiles, 128, eavsr_conv_wgrad_blocks).  127 and 128 tiles: one each; 129: one workgroup
    with two; 256: two each; 257: one with three; 127 tiles of a 506-row image and the two of an 8 x 32 one: the workspace holds
    64 slabs and one, so the second clamp binds.  The bias gradient rides in the launch (its slab lies behind the
    eavsr_conv_wgrad_blocks weight slabs)."""
    from eavsr_amd import ops
    _need_x6(ops)
    assert w % 4 == 0 and n * nseg * _cdiv(h, 4) * _cdiv(w, 32) == tiles
    blocks = ops.lib().eavsr_conv_wgrad_blocks(n * nseg, h, w, 3)
    assert blocks == min(n * nseg * _cdiv(h, 8) * _cdiv(w, 32), MAX_SLABS)
    assert min(tiles, X6_MAX_SLABS, blocks) == slabs
    _exercise(cuda, 3, (12,), 10, (n, h, w), nseg=nseg, scaled=False, entries=("single", "multi1") if nseg == 1 else ("multiN", "multiN_acc"))


# ------------------------------------------------------------------------------------------- 5. degenerate extents
@pytest.mark.parametrize("k,chans,precision", [(1, (12, 5), "fp32"), (1, (72,), "fp32"), (3, (12, 5), "fp32"), (3, (12, 5), "bf16"),
                                               (5, (12, 5), "fp32")], ids=_ids)
def test_empty_batch_gives_zeros_or_leaves_what_was_there(cuda, k, chans, precision):
    """n == 0 through both entry points: zeros (weight and bias) without accumulate, the tensors as they were with it"""
    _exercise(cuda, k, chans, 10, (0, 6, 8), nseg=2, precision=precision)


@pytest.mark.parametrize("shape", [(2, 1, 40), (2, 12, 1), (1, 1, 1), (2, 9, 3), (2, 9, 2), (3, 1, 4)], ids=_ids)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_images_one_pixel_high_or_narrower_than_a_float4(cuda, k, shape):
    """h or w of 1 (every tap but the centre row / column reads padding only) and w < 4; 1 x 40 and 1 x 4 on the bf16x6 kernel"""
    _exercise(cuda, k, (12, 5), 10, shape)


@pytest.mark.parametrize("shape", [(1, 6, 36), (1, 6, 38)], ids=_ids)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_eight_uses_in_one_launch(cuda, k, shape):
    """nseg == WGRAD_MAX_SEGMENTS: every pointer slot of the kernel arguments is a use of its own"""
    from eavsr_amd import ops
    assert ops.WGRAD_MAX_SEGMENTS == 8
    _exercise(cuda, k, (12, 5), 10, shape, nseg=8, entries=("multiN", "multiN_acc"))


# ------------------------------------------------------------------------------------------- 6. the bf16 training precision
@pytest.mark.parametrize("shape", SMALL, ids=_ids)
@pytest.mark.parametrize("chans,cout", [((64,), 3), ((64,), 256), ((256,), 64), ((3,), 64)], ids=_ids)
def test_channel_blocks_in_the_bf16_training_precision(cuda, chans, cout, shape):
    """precision="bf16" where ops.wgrad_bf16_takes holds (conv_wgrad3_x6_kernel<1>): dY and X rounded once to nearest even, the
    same blocks, slabs and fixed-order reduction"""
    _exercise(cuda, 3, chans, cout, shape, precision="bf16")
