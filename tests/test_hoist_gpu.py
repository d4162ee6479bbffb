"""GPU tests of the alignment module in two halves: the offset predictors of a whole branch computed ahead of the recurrence
(`EAVSRP._predict_branch`, `MultiAdSTN.predict`), warp + DCNv2 inside it (`MultiAdSTN.sample`) -- and of the native pieces that
needs: one half of the pair warp as a launch of its own, the 5x5 heads on a stack of images, the heads-mode DCNv2 reading a slice
of that stack.  Everything here is bit for bit: the split reorders launches and batches them, it computes nothing differently.
Run with `pytest -m gpu` on a MI355X."""
from argparse import Namespace

import pytest
import torch

from oracle import eavsr_oracle as O
from tests import helpers as H
from tests.golden import cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda):
    from eavsr_amd import ops as _ops
    _ops.lib()  # fails loudly if the HIP extension is missing
    return _ops


def g(t, dev):
    return t.to(dev).contiguous()


# ------------------------------------------------------------------------------------------ the model, hoisted against per-step
_BRANCHES = ("backward_1", "forward_1", "backward_2", "forward_2")


def _forward_with_branches(net, lrs, ops):
    """(SR output, {branch: frame-major features}, launches of the 5x5 heads) of the real `forward`"""
    seen = {}
    tail = net.upsample

    def upsample(lqs, feats, lq_tm=None):
        for k in _BRANCHES:
            seen[k] = torch.cat(list(feats[k]), 0).clone()
        return tail(lqs, feats, lq_tm)

    net.upsample = upsample
    try:
        with torch.no_grad(), ops.profile() as prof:
            sr = net(lrs)
        names = prof.summary()["conv5x5_64to120_x6"]["calls"]
    finally:
        del net.upsample
    return sr, seen, names


@pytest.mark.parametrize("scale,clips", [(4, 1), (2, 1), (4, 2)])
def test_hoisted_predictors_equal_the_per_step_recurrence(ops, cuda, scale, clips):
    """1 (2) clips x 4 frames x 3 x 64 x 72: the minimum height, a width that is no multiple of the 64- / 32-pixel tiles; four
    frames run the i = 1 (no second order) and the i >= 2 steps in both directions; with 2 clips a row block of the predictor stack
    is not one image.  SR output and all four branches' features: torch.equal."""
    from eavsr_amd import eavsrp_model as M
    from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of, synthetic_clip
    net = M.EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=scale), None)
    sd0 = net.state_dict()
    net.load_state_dict(fill_state_dict(shapes_of(sd0), "trained_like", fixed=sd0), strict=True)
    net = net.to(cuda).eval()
    lrs = synthetic_clip(clips, 4, 64, 72, seed=11).to(cuda)
    prev = M.HOIST_PREDICTORS
    try:
        M.HOIST_PREDICTORS = True
        sr_h, br_h, names_h = _forward_with_branches(net, lrs, ops)
        M.HOIST_PREDICTORS = False
        sr_s, br_s, names_s = _forward_with_branches(net, lrs, ops)
    finally:
        M.HOIST_PREDICTORS = prev
    # each run took the path it is named after: one heads launch per branch, or one per first- / second-order time step (3 + 2)
    assert (names_h, names_s) == (4, 20), (names_h, names_s)
    assert tuple(sr_h.shape) == (clips, 4, 3, 64 * scale, 72 * scale)
    assert torch.isfinite(sr_h).all()
    for k in _BRANCHES:
        assert br_h[k].shape == (4 * clips, 64, 64, 72)
        assert torch.equal(br_h[k], br_s[k]), k
    assert torch.equal(sr_h, sr_s)


def test_predict_then_sample_equals_the_module(ops, cuda):
    """MultiAdSTN.sample(feat_prop, *MultiAdSTN.predict(nbr, cur, flow)) against MultiAdSTN.forward on 2 x 64 x 64 x 72: torch.equal"""
    from eavsr_amd import networks as Nw
    from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of
    m = Nw.MultiAdSTN(Namespace(n_frame=7), 64, 64, deformable_groups=8)
    sd0 = m.state_dict()
    m.load_state_dict(fill_state_dict(shapes_of(sd0), "trained_like", fixed=sd0), strict=True)
    m = m.to(cuda).eval()
    n, h, w = 2, 64, 72
    pyr = lambda seed: [g(cases.randn(seed + i, n, 64, h >> i, w >> i, scale=0.5), cuda) for i in range(3)]
    nbr, cur = pyr(71), pyr(75)
    feat_prop, flow = g(cases.randn(79, n, 64, h, w), cuda), g(cases.randn(80, n, 2, h, w, scale=2.0), cuda)
    with torch.no_grad():
        assert m.can_split(nbr[0], flow)
        want = m(nbr, cur, feat_prop, flow)
        offset, heads = m.predict(nbr, cur, flow)
        assert offset.shape == (n, 2, h, w) and heads.shape == (n, 120, h, w)
        got = m.sample(feat_prop, offset, heads)
    assert torch.isfinite(want).all() and torch.equal(got, want)


# ------------------------------------------------------------------------------------------ one half of the pair warp
@pytest.mark.parametrize("il8", [True, "bf16", "fp16"])
@pytest.mark.parametrize("pad", ["zeros", "border"])
def test_single_warp_il8_equals_the_pair_kernels_second_output(ops, cuda, pad, il8):
    """2 x 64 x 37 x 45 (ragged against the 64 x 4 pixel tile in both directions), flows that leave the image on every side"""
    n, c, h, w = 2, 64, 37, 45
    xa, xb = cases.randn(41, n, c, h, w), cases.randn(42, n, c, h, w)
    flow = cases.randn(43, n, 2, h, w, scale=2.5)
    flow[:, 0, :, :4] -= 9.0          # out on the left, right, top, bottom
    flow[:, 0, :, -4:] += 9.0
    flow[:, 1, :4] -= 7.0
    flow[:, 1, -4:] += 7.0
    flow2 = cases.randn(44, n, 2, h, w, scale=0.7)
    args = (g(flow, cuda), g(flow2, cuda))
    pa, pb = ops.flow_warp_pair(g(xa, cuda), g(xb, cuda), *args, b_il8=il8, padding_mode=pad)
    sb = ops.flow_warp_single(g(xb, cuda), *args, il8=il8, padding_mode=pad)
    assert sb.shape == (n, c // 8, h, w, 8) and sb.dtype == pb.dtype
    assert torch.equal(sb, pb)
    # the other half, which the predictor pass takes -- and against the oracle in both padding modes
    assert torch.equal(ops.flow_warp_single(g(xa, cuda), *args, padding_mode=pad), pa)
    if il8 is True:
        assert H.maxabs(pa.cpu(), O.flow_warp(xa, flow + flow2, pad)) <= 5e-5
    if il8 is True:
        # and the layout holds the warp: against the oracle, tolerance of tests/test_hip_ops.py::test_flow_warp_vs_oracle
        ref = O.flow_warp(xb, flow + flow2, pad)
        assert H.maxabs(sb.cpu().permute(0, 1, 4, 2, 3).reshape(n, c, h, w), ref) <= 5e-5
        # every side was left: some outputs of zeros padding are exact zeros where border padding has values
        assert pad != "zeros" or (ref[:, :, :, 0] == 0).any() and (ref[:, :, :, -1] == 0).any() and (ref[:, :, 0] == 0).any() and (ref[:, :, -1] == 0).any()


# ------------------------------------------------------------------------------------------ the 5x5 heads on a stack of images
def test_heads_conv_on_a_stack_equals_one_launch_per_image(ops, cuda):
    """conv_x6_kernel<5> (64 -> 15 D = 120, the mask sigmoid in its epilogue) on 11 images of 64 x 72 with different contents: one
    launch against 11 launches of one image.  The stack is 132 tiles per output-channel tile, more than one round of workgroups:
    the launch is persistent and a workgroup walks two or more tiles as one stream (the next tile's operands requested under the
    current one's last chunk and epilogue); a single image is one tile per workgroup in the 8-row, 32-channel shape.  Every output
    must be the same sum in the same order in both."""
    D, n, h, w = 8, 11, 64, 72
    f = cases.randn(51, n, 64, h, w, scale=0.5) * torch.arange(1, n + 1).view(n, 1, 1, 1)
    ws = [cases.randn(52, 4 * D, 64, 5, 5, scale=0.01), cases.randn(53, 2 * D, 64, 5, 5, scale=0.02), cases.randn(54, 9 * D, 64, 5, 5, scale=0.03)]
    bs = [torch.tensor([1.0, 0, 0, 1.0]).repeat(D), cases.randn(55, 2 * D, scale=0.5), cases.randn(56, 9 * D, scale=0.5)]
    gw, gb, gf = [g(t, cuda) for t in ws], [g(t, cuda) for t in bs], g(f, cuda)
    assert ops.conv_route(n, h, w, 5, [64], 15 * D, 3, sigmoid_from=6 * D, grad=False).family == "x6"
    with torch.cuda.device(cuda):
        assert ops.lib().eavsr_conv_f32x6_tiles_per_workgroup(n, 64, 15 * D, h, w, 5) >= 2      # some workgroup walks several tiles
        assert ops.lib().eavsr_conv_f32x6_tiles_per_workgroup(1, 64, 15 * D, h, w, 5) == 1
    with torch.no_grad():
        whole = ops.conv2d(gf, gw, gb, sigmoid_from=6 * D)
        each = torch.cat([ops.conv2d(gf[i:i + 1], gw, gb, sigmoid_from=6 * D) for i in range(n)], 0)
    assert whole.shape == (n, 15 * D, h, w)
    assert torch.equal(whole, each)
    assert not torch.equal(whole[0], whole[1])
    m = whole[:, 6 * D:]
    assert (m >= 0).all() and (m <= 1).all() and whole[:, :6 * D].abs().max() > 1      # masks behind channel 6 D, plain values in front


# ------------------------------------------------------------------------------------------ DCNv2 reading a slice of the stack
def test_heads_mode_dcnv2_reads_a_slice_of_the_stacked_heads(ops, cuda):
    """rows 4 .. 5 of a 7-image heads stack (a contiguous frame-major view at a non-zero offset) against a contiguous copy of
    them: bit-equal; against O.dcnv2 on the CPU: the tolerance tests/test_hip_ops.py uses for this kernel"""
    n, h, w, D, rows, first = 2, 13, 37, 8, 7, 4
    c = 8 * D
    x = cases.randn(61, n, c, h, w)
    heads = torch.cat([cases.randn(62, rows, 4 * D, h, w, scale=0.4) + torch.tensor([1.0, 0, 0, 1.0]).repeat(D).view(1, 4 * D, 1, 1),
                       cases.randn(63, rows, 2 * D, h, w, scale=1.5), torch.sigmoid(cases.randn(64, rows, 9 * D, h, w, scale=2.0))], 1)
    wt = cases.randn(65, 64, c, 3, 3, scale=1.0 / (c * 9) ** 0.5)
    b = cases.randn(66, 64, scale=0.1)
    prev = ops.DCN_IL_IMPL
    ops.set_dcn_il_impl("il2")
    try:
        stack = g(heads, cuda)
        view = stack[first:first + n]
        assert view.is_contiguous() and view.data_ptr() != stack.data_ptr()
        xil = ops.to_il8(g(x, cuda))
        out_v = ops.dcnv2_il(xil, view, None, g(wt, cuda), g(b, cuda), D, heads=True, mask_activated=True)
        out_c = ops.dcnv2_il(xil, view.clone(), None, g(wt, cuda), g(b, cuda), D, heads=True, mask_activated=True)
    finally:
        ops.set_dcn_il_impl(prev)
    assert torch.equal(out_v, out_c)
    hs = heads[first:first + n]
    ref = O.dcnv2(x, O.affine_offsets(hs[:, :4 * D], hs[:, 4 * D:6 * D], D), hs[:, 6 * D:], wt, b, 1, 1, 1, 1, D)
    assert H.maxabs(out_v.cpu(), ref) <= 3e-5 * max(1.0, ref.abs().max().item())
