"""Host checks (no GPU) of tests/backward_refs.py: each float64 reference that tests/test_hip_backward_kernels.py differentiates,
run forward, equals the float32 oracle function or aten op it restates; and the sample positions the flow builder makes land in
the regions it promises."""
import pytest
import torch
import torch.nn.functional as F

from oracle import eavsr_oracle as O
from tests import backward_refs as R


def _eq(a64, b32, tol=2e-6):
    a, b = a64.float(), b32.float()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    err = (a - b).abs().max().item()
    assert err <= tol * max(1.0, b.abs().max().item()), err


@pytest.mark.parametrize("hin,win,s", [(12, 20, 0.25), (12, 20, 0.5), (6, 10, 2.0), (4, 20, 0.25)])
def test_resize_reference(hin, win, s):
    x, pre = R.randn64(1, 2, 3, hin, win), R.randn64(2, 2, 3, hin, win)
    hout, wout = int(hin * s), int(win * s)
    post = R.randn64(3, 2, 3, hout, wout)
    want = O._interp_ac((x + pre).float(), s) * s + post.float()
    _eq(R.resize_ac(x, (hout, wout), s, pre, post), want)


def test_flow_warp_reference():
    x = R.randn64(4, 2, 5, 9, 70)
    flow = R.warp_flow(5, 2, 9, 70, "mixed")
    f1 = R.randn64(6, 2, 2, 9, 70, scale=2.0)
    _eq(R.flow_warp(x, f1, flow - f1), O.flow_warp_direct(x.float(), flow.float()), 1e-5)


@pytest.mark.parametrize("D,with_mask", [(1, False), (8, True)])
def test_affine_reference(D, with_mask):
    n, h, w = 2, 5, 7
    heads = R.randn64(7, n, 15 * D if with_mask else 6 * D, h, w)
    off, mask = R.affine(heads, D, with_mask)
    # per pixel and group: offsets (2 x 9) = T (2 x 2) @ R (2 x 9) - R + t, channels g*18 + 2k + {0: y, 1: x}
    T = heads[:, :4 * D].float().reshape(n, D, 2, 2, h, w)
    t = heads[:, 4 * D:6 * D].float().reshape(n, D, 2, 1, h, w)
    Rg = O._REGULAR
    want = torch.einsum("ndijhw,jk->ndikhw", T, Rg) - Rg.view(1, 1, 2, 9, 1, 1) + t
    _eq(off, want.permute(0, 1, 3, 2, 4, 5).reshape(n, 18 * D, h, w))
    if with_mask:
        _eq(mask, torch.sigmoid(heads[:, 6 * D:].float()))
    else:
        assert mask is None


def test_gconv_reference():
    """the two grouped convolutions of the adapt front end, as the oracle writes them"""
    from tests import helpers as H
    sd = H.filled(H.adaptoffset_shapes("f."), "trained_like")
    x, hh = R.randn64(8, 2, 64, 6, 9), R.randn64(9, 2, 64, 6, 9)
    sd64 = {k: v.double() for k, v in sd.items()}
    t = R.gconv(torch.cat([x, hh], 1), sd64["f.concat.0.weight"], sd64["f.concat.0.bias"], "lrelu")
    t = R.gconv(t, sd64["f.concat2.0.weight"], sd64["f.concat2.0.bias"], "lrelu")
    _eq(t, O.adapt_frontend(sd, "f.", x.float(), hh.float()))
    y = R.gconv(x, sd64["f.concat2.0.weight"][:32], None, None)
    _eq(y, F.conv2d(x.float(), sd["f.concat2.0.weight"][:32], None, 1, 1, 1, 32))


def test_pyramid_reference():
    x = R.randn64(10, 2, 3, 8, 12)
    d2, d4 = R.pyramid(x)
    xf = x.float()
    _eq(d2, F.avg_pool2d(xf, 2))
    _eq(d4, F.avg_pool2d(xf[:, :, 1:, 1:], 2, stride=4))      # the inner 2 x 2 of every 4 x 4 block


def test_rcab_tail_reference():
    c, cr = 32, 2
    r, x = R.randn64(11, 2, c, 5, 6), R.randn64(12, 2, c, 5, 6)
    ps = [R.randn64(13, cr, c, 1, 1), R.randn64(14, cr), R.randn64(15, c, cr, 1, 1), R.randn64(16, c)]
    sd = {f"ca.conv_du.{i}.{k}": p.float() for (i, k), p in zip([(0, "weight"), (0, "bias"), (2, "weight"), (2, "bias")], ps)}
    _eq(R.rcab_tail(r, x, *ps), O.ca_layer(sd, "ca.", r.float()) + x.float())


def test_dcnv2_reference():
    n, c, h, w, dg = 1, 16, 6, 9, 2
    x = R.randn64(17, n, c, h, w)
    off = R.dcn_offsets(18, n, dg, h, w, 2.0)
    mask = R.uniform64(19, 0.0, 1.0, n, dg * 9, h, w)
    wt, b = R.randn64(20, 8, c, 3, 3, scale=0.1), R.randn64(21, 8)
    want = O.dcnv2_via_grid_sample(x.float(), off.float(), mask.float(), wt.float(), b.float(), 1, 1, 1, 1, dg)
    _eq(R.dcnv2(x, off, mask, wt, b, dg), want, 1e-5)
    frac = off - torch.floor(off)
    assert ((frac >= 0.05 - 1e-6) & (frac <= 0.95 + 1e-6)).all()


@pytest.mark.parametrize("region", R.REGIONS)
def test_warp_flow_lands_in_its_region(region):
    n, h, w = 2, 7, 70
    flow = R.warp_flow(22, n, h, w, region)
    assert flow.dtype == torch.float64 and torch.equal(flow, flow.float().double())
    tx, ty = R.positions(flow)
    dead, hit = R.no_valid_corner(flow), R.reached(flow)
    fx, fy = tx - torch.floor(tx), ty - torch.floor(ty)
    live = ~dead
    # every sample that has a valid corner sits at least 0.05 away from an integer in both axes
    assert ((fx[live] >= 0.05 - 1e-5) & (fx[live] <= 0.95 + 1e-5) & (fy[live] >= 0.05 - 1e-5) & (fy[live] <= 0.95 + 1e-5)).all()
    in_x, in_y = (tx >= 0) & (tx <= w - 1), (ty >= 0) & (ty <= h - 1)
    if region == "inside":
        assert (in_x & in_y).all() and not dead.any()
    elif region == "edge":
        assert not (in_x & in_y).any() and not dead.any()
        assert ((tx > w - 1) & (tx < w)).any() and ((tx > -1) & (tx < 0)).any()       # only corner column 0 / 1 valid
        assert ((ty > h - 1) & (ty < h)).any() and ((ty > -1) & (ty < 0)).any()
    elif region == "far":
        assert dead.all() and not hit.any()
        assert ((flow[:, 0].abs() > w + 4) | (flow[:, 1].abs() > h + 4)).all()
    else:
        assert (in_x & in_y).float().mean() > 0.4 and dead.any() and (live & ~(in_x & in_y)).any()
    # reached() agrees with a scatter of the bilinear weights of every sample
    x = torch.zeros(n, 1, h, w, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(R.flow_warp(x, flow).sum(), [x])
    assert torch.equal(g[:, 0] > 0, hit)
