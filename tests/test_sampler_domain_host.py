"""The sampler-domain table and references (tests/sampler_domain.py) checked on the host: the float64 references agree with the
oracle's restatements on the finite tiers, the builders cover what they claim to cover, and deliberately wrong samplers are caught
by the very comparisons the GPU tests make."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import c_ref
from oracle import eavsr_oracle as O
from tests import sampler_domain as SD

DCN_SHAPE = (1, 64, 17, 70, 64, 8)


def _dcn_case(tier, shape=(1, 16, 17, 70, 8, 2), seed=0):
    n, c, h, w, cout, dg = shape
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    mask = rng.uniform(0.1, 1.0, (n, dg * 9, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, c, 3, 3)) / (c * 9) ** 0.5).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    off, tag = SD.dcn_offsets(tier, n, dg, h, w, seed)
    return x, off, mask, wt, b, dg, tag


def _finite_only(off):
    """the finite tiers for the restatements that predate the contract: |offset| beyond 2^16 and non-finite entries zeroed"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(off) & (np.abs(off) <= 2.0 ** 16), off, 0).astype(np.float32)


@pytest.mark.parametrize("tier", ["edge", "seam", "wild"])
def test_dcnv2_reference_agrees_with_the_oracles_restatements(tier):
    x, off, mask, wt, b, dg, _ = _dcn_case(tier)
    off = _finite_only(off)
    ref = SD.dcnv2(x, off, mask, wt, b, dg)
    t = [torch.from_numpy(a) for a in (x, off, mask, wt, b)]
    tol = 2e-5 * max(1.0, np.abs(ref).max())
    assert np.abs(O.dcnv2(*t, 1, 1, 1, 1, dg).double().numpy() - ref).max() <= tol
    assert np.abs(c_ref.dcnv2(*t, 1, 1, 1, dg).double().numpy() - ref).max() <= tol


@pytest.mark.parametrize("pad", ["zeros", "border"])
@pytest.mark.parametrize("tier", ["edge", "wild"])
def test_flow_warp_reference_agrees_with_the_oracle_and_grid_sample(tier, pad):
    rng = np.random.RandomState(3)
    x = rng.standard_normal((2, 3, 9, 70)).astype(np.float32)
    flow, _ = SD.warp_flow(tier, 2, 9, 70)
    flow = _finite_only(flow)
    ref, pinned = SD.flow_warp(x, flow, pad)
    assert pinned.all()
    xt, ft = torch.from_numpy(x), torch.from_numpy(flow)
    assert np.abs(O.flow_warp(xt, ft, pad).double().numpy() - ref).max() <= 5e-5
    assert np.abs(c_ref.flow_warp(xt, ft, pad).double().numpy() - ref).max() <= 5e-5
    # torch's own grid_sample at the positions the reference computed (un-normalised by the reference's formula)
    gy, gx = torch.meshgrid(torch.arange(9.0), torch.arange(70.0), indexing="ij")
    grid = torch.stack([2 * (gx + ft[:, 0]) / 69 - 1, 2 * (gy + ft[:, 1]) / 8 - 1], -1)
    gs = F.grid_sample(xt, grid, mode="bilinear", padding_mode=pad, align_corners=True)
    assert np.abs(gs.double().numpy() - ref).max() <= 5e-5


@pytest.mark.parametrize("mode", [("reflection", "bilinear"), ("zeros", "nearest"), ("border", "nearest")])
def test_flow_warp_reference_other_modes_on_the_edge_tier(mode):
    pad, interp = mode
    rng = np.random.RandomState(4)
    x = rng.standard_normal((2, 3, 6, 10)).astype(np.float32)
    flow, _ = SD.warp_flow("edge", 2, 6, 10)
    ref, pinned = SD.flow_warp(x, flow, pad, interpolation=interp)
    assert pinned.all()
    got = O.flow_warp(torch.from_numpy(x), torch.from_numpy(flow), pad, interp).double().numpy()
    if interp == "nearest":      # a tie (position k + 1/2 up to the last ulp of the normalise pair) may round either way
        iy, ix = SD.warp_positions(flow)
        tie = (np.abs(iy - np.floor(iy) - 0.5) < 1e-5) | (np.abs(ix - np.floor(ix) - 0.5) < 1e-5)
        assert tie.mean() < 0.2
        assert np.abs(got - ref)[np.broadcast_to(~tie[:, None], ref.shape)].max() <= 2e-5
    else:
        assert np.abs(got - ref).max() <= 2e-5


@pytest.mark.parametrize("fs", [1, 2])
def test_pwc_backwarp_reference_agrees_with_grid_sample(fs):
    from tests import pwc_ref
    rng = np.random.RandomState(5)
    n, c, h, w = 1, 3, 8, 70
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    flow = _finite_only(SD.pwc_flow("edge", n, h, w, fs))
    (out, mask, ones), (out2, mask2, ones2) = SD.pwc_backwarp(x, flow, fs)
    up = F.interpolate(torch.from_numpy(flow), scale_factor=fs, mode="nearest") if fs > 1 else torch.from_numpy(flow)
    wr = pwc_ref.grid_warp(torch.from_numpy(x), up).double().numpy()
    sure = (np.abs(ones - 0.999) > 1e-5) & (np.abs(ones2 - 0.999) > 1e-5)
    assert sure.mean() > 0.99
    m = (wr[:, -1:] > 0.999)
    assert (m[:, 0][sure] == (mask[:, 0][sure] > 0)).all()
    err = np.minimum(np.abs(wr[:, :-1] * m - out), np.abs(wr[:, :-1] * m - out2))
    assert err[np.broadcast_to(sure[:, None], err.shape)].max() <= 5e-5
    if fs == 1:      # the 0.999 threshold is approached from both sides, closer than 2e-4 and not closer than 1e-5
        near = np.abs(ones - 0.999) < 2e-4
        assert (near & (ones > 0.999)).sum() >= 4 and (near & (ones < 0.999)).sum() >= 4
        assert np.abs(ones - 0.999).min() > 1e-5


# ---- coverage: conditions, not measurements -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["edge", "wild"])
def test_every_table_entry_is_hit_in_every_tap_on_both_axes_from_tile_interior_and_tile_edge(tier):
    n, c, h, w, cout, dg = DCN_SHAPE
    off, tag = SD.dcn_offsets(tier, n, dg, h, w)
    T = len(SD.tier_entries(tier)) + (len(SD.CORNERS) if tier == "edge" else 0)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    edge_px = (yy % SD.TILE_H == 0) | (yy % SD.TILE_H == SD.TILE_H - 1) | (xx % SD.TILE_W == 0) | (xx % SD.TILE_W == SD.TILE_W - 1) | \
              (yy == h - 1) | (xx == w - 1)
    for e in range(1, T + 1):
        for axis in (0, 1):
            hit = tag[..., axis] == e                              # (n, dg, 9, h, w)
            for k in range(9):
                assert hit[:, :, k].any(), (e, axis, k)
            assert (hit & edge_px).any() and (hit & ~edge_px).any(), (e, axis)
    assert (tag == 0).all(-1).mean() >= 0.6                        # the mixed cases stay mostly ordinary
    # and the offsets really put the entries where the table says
    py, px = SD.dcn_positions(off, dg)
    for e, entry in enumerate(SD.tier_entries(tier)):
        for axis, (p, size) in enumerate(((py, h), (px, w))):
            got = p[tag[..., axis] == e + 1]
            if entry[0] == "pos":
                assert (got == np.float32(entry[1] + entry[2] * size)).all(), entry
            elif np.isnan(entry[1]):
                assert np.isnan(got).all()
            elif np.isinf(entry[1]):
                assert (got == entry[1]).all()
            else:
                assert (np.abs(got - entry[1]) <= 128 + abs(entry[1]) * 2.0 ** -23).all(), entry


def test_warp_flow_covers_the_tables():
    for tier in ("edge", "wild"):
        _, tag = SD.warp_flow(tier, 1, 9, 70)
        T = len(SD.tier_entries(tier)) + (len(SD.CORNERS) if tier == "edge" else 0)
        for e in range(1, T + 1):
            assert (tag[..., 0] == e).any() and (tag[..., 1] == e).any(), (tier, e)
        assert (tag == 0).all(-1).mean() >= 0.6


def test_seam_entries_land_on_the_intended_side_of_the_window_test():
    n, c, h, w, cout, dg = DCN_SHAPE
    off, tag = SD.dcn_offsets("seam", n, dg, h, w)
    py, px = SD.dcn_positions(off, dg)
    plan = SD.seam_plan(h, w)
    seen = set()
    for i, (wname, y, x, axis, slot, fl, frac) in enumerate(plan):
        k, g = i % 9, (i // 9) % dg
        if tag[0, g, k, y, x, axis] != 1 + SD.SEAM_SLOTS.index(slot) + (4 if wname == "ws" else 0):
            continue                                                # (a later placement took this slot)
        win = SD.WINDOWS[wname]
        y0, x0 = y // SD.TILE_H * SD.TILE_H, x // SD.TILE_W * SD.TILE_W
        p = (py, px)[axis][0, g, k, y, x]
        assert p == np.float32(fl + frac) and -1 < p < (h, w)[axis] - 1
        fast = bool(SD.in_window(np.floor(py[0, g, k, y, x]), np.floor(px[0, g, k, y, x]), y0, x0, win))
        assert fast == (slot in ("first", "last")), (wname, y, x, axis, slot)
        my, mx, ph, pw = win
        r = fl - ((y0 - my) if axis == 0 else (x0 - mx))
        assert r == {"before": -1, "first": 0, "last": (ph, pw)[axis] - 2, "after": (ph, pw)[axis] - 1}[slot]
        seen.add((wname, axis, slot, frac, (y, x)[axis] == (y0, x0)[axis]))
    for wname in ("il", "ws"):
        for axis in (0, 1):
            for slot in SD.SEAM_SLOTS:
                for frac in (0.0, 0.5):
                    assert any(s[:4] == (wname, axis, slot, frac) for s in seen), (wname, axis, slot, frac)
                assert {s[4] for s in seen if s[:3] == (wname, axis, slot)} == {True, False}, (wname, axis, slot)


def test_all_invalid_builder_leaves_the_bias():
    x, off, mask, wt, b, dg, _ = _dcn_case("edge", (1, 16, 9, 33, 8, 2))
    pixels = [(0, 0), (3, 7), (8, 32), (4, 31)]
    off2 = SD.dcn_all_invalid(off, 9, 33, pixels)
    py, px = SD.dcn_positions(off2, dg)
    gate = SD.dcn_gate(py, px, 9, 33)
    out = SD.dcnv2(x, off2, mask, wt, b, dg)
    for (y, xx) in pixels:
        assert not gate[:, :, :, y, xx].any()
        assert (out[0, :, y, xx] == b.astype(np.float64)).all()
    f2 = SD.warp_all_invalid(SD.warp_flow("ordinary", 1, 9, 33)[0], pixels)
    o, _ = SD.flow_warp(x, f2)
    for (y, xx) in pixels:
        assert (o[0, :, y, xx] == 0).all()


# ---- deliberately wrong samplers must be caught by the GPU tests' own comparisons ----------------------------------------------------
def _fwd_detects(tier, variant, shape=(1, 16, 17, 70, 8, 2), **kw):
    x, off, mask, wt, b, dg, _ = _dcn_case(tier, shape)
    ref = SD.dcnv2(x, off, mask, wt, b, dg)
    bad = SD.dcnv2(x, off, mask, wt, b, dg, variant, **kw)
    assert np.isfinite(ref).all()
    err = np.abs(bad - ref)
    return not (np.nan_to_num(err, nan=np.inf).max() <= 3e-5 * max(1.0, np.abs(ref).max()))


def test_a_nan_position_taken_as_index_0_is_caught():
    assert _fwd_detects("wild", "nan0")
    assert not _fwd_detects("wild", None)


def test_a_wrapping_conversion_is_caught():
    assert _fwd_detects("wild", "wrap")


@pytest.mark.parametrize("win", ["il", "ws"])
def test_a_seam_off_by_one_is_caught(win):
    assert _fwd_detects("seam", "seam", tile_window=SD.WINDOWS[win])


def test_a_gate_inclusive_at_size_is_the_same_function():
    """p = size has BOTH corners of that axis (size, size + 1) outside the image: value, dx, dmask and doffset are exactly 0 with the
    gate `p < size` and with `p <= size` alike -- the two gates are one function and no comparison can (or need) tell them apart.
    Pinned here so that the claim is checked, not assumed: every output of the backward reference is identical under either gate."""
    x, off, mask, wt, b, dg, _ = _dcn_case("edge")
    dy = np.random.RandomState(9).standard_normal((1, 8, 17, 70))
    py, px = SD.dcn_positions(off, dg)
    assert (py == 17).any() and (px == 70).any()
    good, bad = SD.dcnv2_backward(x, off, mask, wt, dy, dg), SD.dcnv2_backward(x, off, mask, wt, dy, dg, "gate_le")
    for a, b_ in zip(good[:3], bad[:3]):
        assert np.array_equal(a, b_)
    assert np.array_equal(SD.dcnv2(x, off, mask, wt, b, dg), SD.dcnv2(x, off, mask, wt, b, dg, "gate_le"))


@pytest.mark.parametrize("variant", ["gate_ge"])
def test_an_inclusive_gate_is_caught_by_the_exact_zeros_of_doffset(variant):
    """p = -1 samples zero either way (the in-image corner has weight 0): the forward cannot tell `<` from `<=`.  The gate
    shows in doffset, which is exactly 0 at a gate-invalid sample and the one-sided slope otherwise."""
    x, off, mask, wt, b, dg, _ = _dcn_case("edge")
    rng = np.random.RandomState(9)
    dy = rng.standard_normal((1, 8, 17, 70))
    _, doff, _, ok = SD.dcnv2_backward(x, off, mask, wt, dy, dg)
    _, bad, _, _ = SD.dcnv2_backward(x, off, mask, wt, dy, dg, variant)
    py, px = SD.dcn_positions(off, dg)
    invalid = np.repeat(~SD.dcn_gate(py, px, 17, 70), 2, axis=2).reshape(doff.shape)      # (n, dg, 9 -> 18, h, w)
    assert (doff[invalid] == 0).all()
    assert (bad[invalid] != 0).any()
    assert not _fwd_detects("edge", variant)      # (documented: invisible to the forward)


def test_backward_reference_agrees_with_autograd_of_the_oracle():
    x, off, mask, wt, b, dg, _ = _dcn_case("edge", (1, 16, 9, 33, 8, 2))
    rng = np.random.RandomState(11)
    dy = rng.standard_normal((1, 8, 9, 33)).astype(np.float32)
    dx, doff, dmask, ok = SD.dcnv2_backward(x, off, mask, wt, dy, dg)
    lv = [torch.from_numpy(a).double().requires_grad_(True) for a in (x, off, mask)]
    out = O.dcnv2(lv[0], lv[1], lv[2], torch.from_numpy(wt).double(), torch.from_numpy(b).double(), 1, 1, 1, 1, dg)
    gx, go, gm = torch.autograd.grad((out * torch.from_numpy(dy).double()).sum(), lv)
    # (the float64 oracle adds pixel + offset in float64, the reference rounds the position to fp32 as the kernels do: <= 2^-18 at
    # these sizes, times gradients of order 1)
    assert np.abs(gx.numpy() - dx).max() <= 2e-5 and np.abs(gm.numpy() - dmask).max() <= 2e-5
    assert (np.abs(go.numpy() - doff) > 2e-5 * max(1.0, np.abs(doff).max()))[ok].mean() <= 0.002
    # flow_warp
    flow, _ = SD.warp_flow("edge", 1, 9, 33)
    g = rng.standard_normal((1, 16, 9, 33)).astype(np.float32)
    dxw, dfl, okw, _ = SD.flow_warp_backward(x, flow, g)
    lw = [torch.from_numpy(x).requires_grad_(True), torch.from_numpy(flow).requires_grad_(True)]
    o = O.flow_warp(lw[0], lw[1], "zeros")
    tx, tf = torch.autograd.grad((o * torch.from_numpy(g)).sum(), lw)
    assert np.abs(tx.numpy() - dxw).max() <= 1e-4 * max(1.0, np.abs(dxw).max())
    bad = (np.abs(tf.numpy() - dfl) > 2e-4 * max(1.0, np.abs(dfl).max()))[okw].mean()
    assert bad <= 0.01      # fp32 floor() of the oracle may take the other side at a handful of near-integer positions


def test_heads_expansion_overflows_to_inf_from_finite_heads():
    """T = 3e38: T0 ry + T1 rx overflows at the diagonal taps -> offsets +-inf from finite heads, fractions inf - inf = NaN in a
    sampler that does not clamp; a non-finite head gives NaN offsets (inf x 0) at the centre row / column"""
    D, h, w = 2, 4, 5
    heads = np.zeros((1, 15 * D, h, w), np.float32)
    heads[:, 0:4 * D:4] = 1.0
    heads[:, 3:4 * D:4] = 1.0
    heads[:, 0:4, 1, 1] = 3e38
    heads[:, 0, 2, 2] = np.inf
    off, m = SD.heads_offsets(heads, D)
    o = off.reshape(1, D, 9, 2, h, w)
    assert np.isfinite(heads[:, :, 1, 1]).all() and np.isinf(o[0, 0, 0, 0, 1, 1]) and np.isinf(o[0, 0, 8, 0, 1, 1])
    assert np.isnan(o[0, 0, 4, 0, 2, 2])
    assert (o[0, 1] == 0).all() and (o[0, 0, :, :, 0, 0] == 0).all()


@pytest.mark.parametrize("tier", ["edge", "seam"])
def test_heads_with_identity_transform_reproduce_the_table_positions(tier):
    n, c, h, w, cout, dg = DCN_SHAPE
    off, tag = SD.dcn_offsets(tier, n, dg, h, w)
    heads, k = SD.heads_from_offsets(off, tag, dg)
    got, _ = SD.heads_offsets(heads, dg)
    want = np.take_along_axis(off.reshape(n, dg, 9, 2, h, w), k[:, :, None, None], axis=2)      # the chosen tap's offset, at every tap
    assert np.array_equal(got.reshape(n, dg, 9, 2, h, w), np.broadcast_to(want, (n, dg, 9, 2, h, w)))
    tagged = (tag != 0).any(-1)
    chosen = np.take_along_axis(tagged, k[:, :, None], axis=2)[:, :, 0]
    assert (chosen == tagged.any(2)).all() and chosen.sum() >= (1000 if tier == "edge" else 50)
