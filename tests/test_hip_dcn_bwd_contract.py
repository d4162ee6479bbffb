"""The sampler-side DCNv2 backward (csrc/dcn_bwd.hip, eavsr_dcnv2_bwd_f32) held to its contract (tests/dcn_bwd_contract.py,
DESIGN.md 4c), element by element:

  1. |out - fp64| <= gamma(c) A for dx, doffset, dmask and dweight at EVERY element, on every case x offset field x value field
  2. exact zero where A = 0: behind a zero dy, off every touched cell, and dweight[co' != co] of a one-hot dy
  3. need_dx=False, accumulate=True and a recycled workspace change nothing they should not
  4. dcnv2_col2im, dcnv2_col2im_dx_det and dcnv2_im2col on the same fields, held to the same bound without the GEMM term

EAVSR_DCNB_CONTRACT_REPORT=<file> appends the measured figures as JSON lines (profiles/r34_dcn_bwd_contract.json was collected
that way)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import dcn_bwd_contract as B
from tests import sampler_domain as SD

pytestmark = pytest.mark.gpu


def _report(**row):
    path = os.environ.get("EAVSR_DCNB_CONTRACT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


@pytest.fixture(scope="module")
def ops(cuda):
    from eavsr_amd import ops as _ops
    _ops.lib()      # fails loudly if the HIP extension is missing
    return _ops


def t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)      # (a copy: the cached inputs are read-only)


def run(ops, dev, v, **kw):
    with ops.profile() as prof:
        dx, doff, dmask, dw = ops.dcnv2_bwd(t(v["x"], dev), t(v["off"], dev), t(v["mask"], dev), t(v["wt"], dev), t(v["dy"], dev), B.DG, **kw)
    assert "dcnv2_bwd" in prof.summary() and not ({"dcnv2_im2col", "dcnv2_col2im"} & set(prof.summary())), list(prof.summary())
    return dict(dx=None if dx is None else dx.cpu().numpy(), doff=doff.cpu().numpy(), dmask=dmask.cpu().numpy(), dw=dw.cpu().numpy())


def test_grid_is_the_restated_one(ops):
    for cs in B.CASES:
        assert int(ops.lib().eavsr_dcnv2_bwd_grid(cs.n, cs.h, cs.w)) == cs.geo.grid, cs


@pytest.mark.parametrize("vf", B.VALUE_FIELDS)
@pytest.mark.parametrize("of", B.OFFSET_FIELDS)
@pytest.mark.parametrize("cid", [c.id for c in B.CASES])
def test_local_bound(ops, cuda, cid, of, vf):
    v, r = B.inputs(cid, of, vf)
    got = run(ops, cuda, v)
    olds = {k: B.old_metric(got[k], ref) for k, ref, _ in r.pairs()}
    err = {k: float(np.abs(got[k].astype(np.float64) - ref).max()) for k, ref, _ in r.pairs()}
    print(f"{cid}/{of}/{vf}: max err {err} old metric {olds}")
    ratios = B.check_all(got, r, f"{cid}/{of}/{vf}")      # (raises with the worst element; frac_ok all true: nothing is excluded)
    print(f"{cid}/{of}/{vf}: err/bound {ratios}")
    _report(test="local", case=cid, offsets=of, values=vf, ratio=ratios, old=olds)


@pytest.mark.parametrize("of", B.OFFSET_FIELDS)
@pytest.mark.parametrize("cid", [c.id for c in B.CASES])
def test_exact_zero_locality(ops, cuda, cid, of):
    """`masked` dy: doffset / dmask are +-0 at every pixel whose dy is 0 in all 64 channels, dx at every cell no sample of a non-zero
    pixel touches (A = 0 says both), dweight where the modulation mask of the group is 0"""
    v, r = B.inputs(cid, of, "masked")
    got = run(ops, cuda, v)
    n, h, w = v["x"].shape[0], v["x"].shape[2], v["x"].shape[3]
    dead = ~(v["dy"] != 0).any(axis=1)                                         # (n, h, w)
    assert 0 < dead.mean() < 1
    assert (got["doff"][np.broadcast_to(dead[:, None], got["doff"].shape)] == 0).all()
    assert (got["dmask"][np.broadcast_to(dead[:, None], got["dmask"].shape)] == 0).all()
    # cells touched by a sample of a live pixel, from the geometry (not from the bound)
    s = B.sample_geometry(v["off"], B.case(cid).geo)
    live = s["gate"] & np.broadcast_to(~dead[:, None, None], s["gate"].shape) & (v["mask"].reshape(n, B.DG, 9, h, w) != 0)
    touched = np.zeros((n, B.DG, h, w), bool)
    nn, gg = np.nonzero(live)[0], np.nonzero(live)[1]
    for d in (0, 1):
        for e in (0, 1):
            cy, cx = s["fy"][live] + d, s["fx"][live] + e
            ok = (cy >= 0) & (cy < h) & (cx >= 0) & (cx < w)
            touched[nn[ok], gg[ok], cy[ok], cx[ok]] = True
    quiet = np.repeat(~touched, B.CPG, axis=1)
    assert quiet.any() and (r.b_dx[quiet] == 0).all() and (r.b_dx[~quiet] > 0).all()
    stray = (got["dx"] != 0) & quiet
    assert not stray.any(), f"{int(stray.sum())} non-zero dx cells that nothing touches, first at {tuple(np.argwhere(stray)[0])}"
    zero_w = np.zeros((64, B.DG, B.CPG, 3, 3), bool)
    zero_w[:, list(B.MASKED_ZERO_GROUPS)] = True
    assert (got["dw"].reshape(zero_w.shape)[zero_w] == 0).all()
    _report(test="zeros", case=cid, offsets=of, dx_cells=int(quiet.sum()), pixels=int(dead.sum()))


def test_one_hot_dy_leaves_the_other_output_channels_zero(ops, cuda):
    """one pixel, one channel: walked over the first and last pixel of every wave row of a straddling workgroup's two units"""
    cs = B.case("per2_straddle")
    geo = cs.geo
    v, _ = B.inputs(cs.id, "noise", "noise")
    col = SD.dcn_columns(v["x"], v["off"], v["mask"], B.DG)                    # (1, 64, 9, h, w)
    acol = SD.dcn_columns(np.abs(v["x"]), v["off"], np.abs(v["mask"]), B.DG)   # the same on absolute values: a sample's corners cancel
    b = geo.straddlers()[0]
    checked, worst = 0, 0.0
    for i, u in enumerate(geo.wg_units(b)):
        _, bn, ty, tx = geo.unit(u)
        for wv in range(4):
            for x in (tx * 16, min(tx * 16 + 15, cs.w - 1)):
                y, co = ty * 4 + wv, (7 * checked + 3) % 64
                vv = dict(v)
                dy = np.zeros_like(v["dy"])
                dy[bn, co, y, x] = 1.5
                vv["dy"] = dy
                dw = run(ops, cuda, vv, need_dx=False)["dw"]
                others = np.delete(dw, co, axis=0)
                assert (others == 0).all(), (u, y, x, co, int((others != 0).sum()))
                ref = 1.5 * col[bn, :, :, y, x].reshape(64, 3, 3)
                # one addend per element: the sample's 8 roundings and one accumulate inside the matrix instruction (2 u); every
                # other addition adds an exact zero
                worst = max(worst, B.check_local(dw[co], ref, B.gamma(B.C0_DW + 2) * 1.5 * acol[bn, :, :, y, x].reshape(64, 3, 3),
                                                   f"one-hot {u, y, x}"))
                checked += 1
    assert checked == 16
    print("one-hot: largest err/bound", worst)
    _report(test="one_hot", launches=checked, ratio=worst)


def test_modes(ops, cuda):
    v, r = B.inputs("per2_straddle", "far", "noise")
    full = run(ops, cuda, v)
    B.check_all(full, r, "full")
    # need_dx=False: the same DATA and WGT instantiations, bit for bit
    nodx = run(ops, cuda, v, need_dx=False)
    assert nodx["dx"] is None
    for k in ("doff", "dmask", "dw"):
        assert np.array_equal(full[k].view(np.uint32), nodx[k].view(np.uint32)), k
    # accumulate=True onto a known tensor: that tensor plus the plain result, one rounding per element
    base = np.random.RandomState(5).standard_normal((64, 64, 3, 3)).astype(np.float32)
    acc = t(base, cuda)
    out = ops.dcnv2_bwd(t(v["x"], cuda), t(v["off"], cuda), t(v["mask"], cuda), t(v["wt"], cuda), t(v["dy"], cuda), B.DG, need_dx=False,
                        dweight=acc, accumulate=True)
    assert out[3] is acc
    want = base.astype(np.float64) + full["dw"].astype(np.float64)
    assert (np.abs(acc.cpu().numpy().astype(np.float64) - want) <= B.U * np.abs(want)).all()
    # accumulate=False into a given tensor overwrites it
    ops.dcnv2_bwd(t(v["x"], cuda), t(v["off"], cuda), t(v["mask"], cuda), t(v["wt"], cuda), t(v["dy"], cuda), B.DG, need_dx=False, dweight=acc)
    assert np.array_equal(acc.cpu().numpy().view(np.uint32), full["dw"].view(np.uint32))


def test_stale_workspace_contents_do_not_matter(ops, cuda):
    """the workspace, doffset and dmask come from torch.empty: blocks of their sizes are filled with a large finite value and freed,
    so the caching allocator hands the next call exactly those -- which is checked, not assumed"""
    cs = B.case("per3_splits")
    v, r = B.inputs(cs.id, "seams", "blocks")
    first = run(ops, cuda, v)
    ws = int(ops.lib().eavsr_dcnv2_bwd_workspace_floats(cs.n, cs.h, cs.w))
    # every block a call takes: the uploads and the outputs share sizes (offset / doffset, mask / dmask, x / dy / IL8 copies / dx)
    sizes = (ws,) + 2 * (v["off"].size,) + 2 * (v["mask"].size,) + 6 * (v["x"].size,) + 2 * (64 * 64 * 9,)

    def junk():
        blocks = [torch.full((k,), 3.0e38, device=cuda) for k in sizes]
        torch.cuda.synchronize()
        del blocks

    junk()
    again = [torch.empty(k, device=cuda) for k in sizes]      # what the call's own torch.empty would get
    reused = [bool((a == 3.0e38).all()) for a in again]
    del again
    assert all(reused), reused      # the junk came back, block for block
    junk()
    second = run(ops, cuda, v)
    for k in ("doff", "dmask", "dw"):
        assert np.array_equal(first[k].view(np.uint32), second[k].view(np.uint32)), k
    # dx: this field sends samples down the atomic path, whose order is free -- held to the bound, not to the first call's bits
    B.check_all(second, r, "after junk")


@pytest.mark.parametrize("of", ["seams", "converge", "far"])
@pytest.mark.parametrize("cid", ["per1_ragged", "per2_ragged"])
def test_column_path_agrees(ops, cuda, cid, of):
    """im2col's columns, col2im (atomic) and the deterministic dx, fed the fp64 column gradient rounded once to fp32"""
    v, r0 = B.inputs(cid, of, "blocks")
    n, c, h, w = v["x"].shape
    dcol = np.einsum("ok,nop->nkp", v["wt"].reshape(64, 576).astype(np.float64), v["dy"].reshape(n, 64, h * w).astype(np.float64))
    dcol = dcol.reshape(n, 576, h, w).astype(np.float32)
    r = B.reference(v["x"], v["off"], v["mask"], v["wt"], None, dcol=dcol, gemm=False, want_col=True)
    assert r.frac_ok.all()
    g = lambda k: t(v[k], cuda)
    col = ops.dcnv2_im2col(g("x"), g("off"), g("mask"), B.DG).cpu().numpy()
    ratios = dict(col=B.check_local(col.reshape(r.col.shape), r.col, r.b_col, "columns"))
    dx, doff, dmask = ops.dcnv2_col2im(g("x"), g("off"), g("mask"), t(dcol, cuda), B.DG)
    ratios.update(B.check_all(dict(dx=dx.cpu().numpy(), doff=doff.cpu().numpy(), dmask=dmask.cpu().numpy()), r, "col2im"))
    det = ops.dcnv2_col2im_dx_det(g("off"), g("mask"), t(dcol, cuda), B.DG).cpu().numpy()
    ratios["dx_det"] = B.check_local(det, r.dx, r.b_dx, "dx_det")
    print(f"{cid}/{of}: err/bound {ratios}")
    _report(test="columns", case=cid, offsets=of, ratio=ratios)
