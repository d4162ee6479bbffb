"""Host side of the contract of the sampler-side DCNv2 backward (tests/dcn_bwd_contract.py): the restated geometry has
the properties the case table claims, the offset fields reach what they aim at, the reference is the float64 autograd of the
oracle, the fp32 emulation stays inside the per-element bound -- and every mutant of the emulation is rejected by the new
checks, most of them on inputs where the old global metric accepts them.  No GPU."""
import numpy as np
import pytest
import torch

from tests import dcn_bwd_contract as B


def _emulate(cid, of, vf, **kw):
    v, r = B.inputs(cid, of, vf)
    return B.emulate32(v["x"], v["off"], v["mask"], v["wt"], v["dy"], **kw), r


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def test_case_table_has_the_unit_counts_it_claims():
    per = {c.id: c.geo.per for c in B.CASES}
    assert per == {"per1_ragged": 1, "per2_straddle": 2, "per2_ragged": 2, "per2_images": 2, "per2_two_images": 2, "per3_splits": 3}
    assert [c.geo.ntiles for c in B.CASES] == [8, 65, 65, 70, 75, 133]
    for c in B.CASES:
        g = c.geo
        assert g.grid == min(g.total, 512) and g.per * g.grid >= g.total > (g.per - 1) * g.grid
        assert g.per <= g.ntiles and 16 * g.per <= 64      # two groups per workgroup at most; the dweight count's matrix-instruction term
    assert max(c.n * c.h * c.w * 64 for c in B.CASES) == 64 * 28 * 304
    # ragged: waves without pixels, a ragged last tile column
    g = B.case("per1_ragged").geo
    assert g.tiles_y * B.TH - 7 == 1 and g.tiles_x * B.TW - 21 == 11 and g.straddlers() == []
    # 65 tiles, per = 2: every odd group boundary falls inside a workgroup, the other workgroups hold two units of one group
    for cid in ("per2_straddle", "per2_ragged"):
        g = B.case(cid).geo
        st = g.straddlers()
        assert [g.wg_groups(b) for b in st] == [[0, 1], [2, 3], [4, 5], [6, 7]]
        assert all(len(g.wg_units(b)) == 2 for b in range(g.total // 2)) and len(g.wg_groups(0)) == 1
    assert B.case("per2_ragged").h % B.TH and B.case("per2_ragged").w % B.TW
    # 70 tiles: group boundaries aligned with the workgroups; 14 tiles per image is even, so no workgroup of two holds two images
    g = B.case("per2_images").geo
    assert g.straddlers() == [] and g.per_img == 14
    assert all(len({g.unit(u)[1] for u in g.wg_units(b)}) <= 1 for b in range(g.grid))
    # 25 tiles per image: workgroups whose two units lie in different images -- inside one group (the windows, the image index and
    # the dW accumulators go from one image to the next) and across a group boundary (the last image's last tile, then image 0)
    g = B.case("per2_two_images").geo
    assert g.per_img == 25 and g.n == 3
    mixed = [b for b in range(g.grid) if len({g.unit(u)[1] for u in g.wg_units(b)}) == 2]
    assert 12 in mixed and [g.unit(u)[:2] for u in g.wg_units(12)] == [(0, 0), (0, 1)]
    assert len([b for b in mixed if b not in g.straddlers()]) >= 8 and set(g.straddlers()) <= set(mixed) and len(g.straddlers()) == 4
    assert [g.unit(u)[:2] for u in g.wg_units(g.straddlers()[0])] == [(0, 2), (1, 0)]
    g = B.case("per3_splits").geo
    splits = set()
    for b in g.straddlers():
        us = [u // g.ntiles for u in g.wg_units(b)]
        splits.add((us.count(us[0]), us.count(us[-1])))
    assert splits == {(1, 2), (2, 1)}
    assert g.grid == 512 and sum(1 for b in range(g.grid) if len(g.wg_units(b)) == 0) > 0      # idle trailing workgroups


def test_slot_rule_matches_the_order_in_which_a_workgroup_meets_its_groups():
    for c in B.CASES:
        g = c.geo
        for b in range(g.grid):
            for i, grp in enumerate(g.wg_groups(b)):
                assert g.slot(b, grp) == i and b in g.wgs_of_group(grp)
        for grp in range(B.DG):
            assert [b for b in range(g.grid) if grp in g.wg_groups(b)] == list(g.wgs_of_group(grp))


def test_gather_ranges_cover_exactly_the_slabs_that_hold_a_cell():
    g = B.case("per2_straddle").geo
    for y in range(g.h):
        for x in (0, 7, 8, 23, 24, 100, g.w - 1):
            want = [(ty, tx) for ty in range(g.tiles_y) for tx in range(g.tiles_x)
                    if 0 <= y - (B.TH * ty - B.WY) < B.UH and 0 <= x - (B.TW * tx - B.WX) < B.WW]
            assert g.gather_tiles(y, x) == want
            rows = sorted({t[0] for t in want})
            if 6 <= y <= g.h - 10:      # a 16-row slab every 4 rows: four tile rows hold an interior cell ...
                assert len(rows) == 4
            # ... and the first of them holds it in its LAST slab row, which only wave 3's window row 12 fills, exactly at y = 1 (mod 4)
            assert (y - (B.TH * rows[0] - B.WY) == B.UH - 1) == (y % 4 == 1 and y >= 9)


def test_tap_pairing():
    assert [(B.b_tap(mt, 0), B.b_tap(mt, 1)) for mt in range(B.MT)] == [(0, 5), (1, 6), (2, 7), (3, 8), (4, 9)]
    assert all(abs(a // 3 - b // 3) >= 1 for a, b in [(0, 5), (1, 6), (2, 7), (3, 8)])      # at least one filter row apart


# ---- the offset fields -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("of", B.OFFSET_FIELDS)
@pytest.mark.parametrize("cs", B.CASES, ids=lambda c: c.id)
def test_no_position_is_an_integer(cs, of):
    s = B.sample_geometry(B.offsets(cs, of), cs.geo)
    for p in (s["py"], s["px"]):
        assert set(np.unique(p - np.floor(p)).tolist()) <= {0.25, 0.5, 0.75}
    assert s["nonint"].all()


@pytest.mark.parametrize("cs", B.CASES, ids=lambda c: c.id)
def test_seam_field_reaches_every_slot(cs):
    s = B.sample_geometry(B.offsets(cs, "seams"), cs.geo)
    plan = B.seam_plan(cs)
    seen = set()
    for p in plan:
        i = (p["bn"], p["g"], p["k"], p["y"], p["x"])
        assert s["gate"][i]
        got = (s["by"][i], s["bx"][i])[p["axis"]]
        assert got == p["slot"], (p, got)
        inside = p["slot"] in ((0, B.WH - 2) if p["axis"] == 0 else (0, B.WW - 2))
        assert bool(s["fast"][i]) == inside, p
        seen.add((p["axis"], p["slot"]))
    assert len({(p["bn"], p["g"], p["k"], p["y"], p["x"]) for p in plan}) == len(plan)
    rows = {(0, r) for r in B.SEAM_ROWS} if cs.h >= 18 else {(0, 0), (0, B.WH - 2)}      # h = 7: rows -1 and 12 leave the image
    cols = {(1, c) for c in B.SEAM_COLS} if cs.w >= 80 else {(1, -1), (1, 0)}      # w = 21: columns 30 / 31 leave the image
    assert seen == rows | cols, seen
    for bn in range(cs.n if cs.w >= 80 else 0):      # every tile and wave row carries placements (7 x 21: nothing fits around tile column 0)
        assert {(p["ty"], p["tx"], p["wave"]) for p in plan if p["bn"] == bn} == \
            {(ty, tx, wv) for ty in range(cs.geo.tiles_y) for tx in range(cs.geo.tiles_x) for wv in range(4) if ty * 4 + wv < cs.h}


@pytest.mark.parametrize("cs", B.CASES, ids=lambda c: c.id)
def test_converge_field_has_every_multiplicity_and_a_chain(cs):
    off = B.offsets(cs, "converge")
    mult = set(B.multiplicities(off, cs.geo).tolist())
    assert {2, 3, 16, 17, 32} <= mult and max(mult) == 32, mult
    assert max(B.multiplicities(B.offsets(cs, "noise"), cs.geo).tolist()) <= 8      # what noise offsets give
    s = B.sample_geometry(off, cs.geo)
    chains = [p for p in B.converge_plan(cs) if p["kind"] == "chain"]
    assert chains
    for p in chains:
        gy, x0 = p["ty"] * 4 + p["wave"], p["tx"] * 16
        fx = s["fx"][p["bn"], p["g"], p["mt"], gy, x0:x0 + 16]
        assert (np.diff(fx) == 1).all() and s["fast"][p["bn"], p["g"], p["mt"], gy, x0:x0 + 16].all()
        assert (s["fy"][p["bn"], p["g"], p["mt"], gy, x0:x0 + 16] == p["fy"]).all()


@pytest.mark.parametrize("cs", B.CASES, ids=lambda c: c.id)
def test_far_field_leaves_the_window_and_fills_four_tile_rows(cs):
    off = B.offsets(cs, "far")
    s = B.sample_geometry(off, cs.geo)
    atomic = s["gate"] & ~s["fast"]
    if cs.h >= 18:
        assert atomic.mean() >= 0.1
        d = np.maximum(np.abs(s["fy"] - s["yy"]) / 4.0, np.abs(s["fx"] - s["xx"]) / 16.0)[atomic]
        assert d.min() >= 1.5 and (d >= 2).mean() > 0.9 and d.max() <= 3.25      # 2 - 3 tiles away
        cov = B.tile_row_coverage(off, cs.geo)
        assert {(1, 0), (1, 3)} <= cov, cov      # a y = 1 (mod 4) cell filled from the first and from the fourth tile row of its gather
    assert (s["fy"][s["gate"]] >= -1).all() and s["gate"].mean() > 0.85


# ---- reference -------------------------------------------------------------------------------------------------------------------
def test_reference_is_the_float64_autograd_of_the_oracle():
    from oracle import eavsr_oracle as O
    v, r = B.inputs("per1_ragged", "noise", "noise")
    t = {k: torch.from_numpy(np.array(a)).double().requires_grad_(k != "dy") for k, a in v.items()}
    out = O.dcnv2(t["x"], t["off"], t["mask"], t["wt"], None, 1, 1, 1, 1, B.DG)
    out.backward(t["dy"])
    for name, ref, tn in (("dx", r.dx, "x"), ("doff", r.doff, "off"), ("dmask", r.dmask, "mask"), ("dw", r.dw, "wt")):
        g = t[tn].grad.numpy()
        assert np.abs(g - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), name
    assert r.frac_ok.all()
    # the bound has no absolute term and is a property of the element
    for _, ref, b in r.pairs():
        assert (b >= 0).all() and (np.abs(ref)[b == 0] == 0).all()


def test_bound_constants_are_the_counted_ones():
    assert (B.C_GEMM, B.C0_DX, B.C0_DMASK, B.C0_DOFF, B.C0_DW, B.C0_COL) == (128, 3 + 1 + 1 + 4 + 8, 7 + 1 + 4 + 1, 4 + 1 + 1 + 4 + 1, 7 + 1, 7 + 1)
    assert B.U == 2.0 ** -24 and abs(B.gamma(100) / (100 * B.U) - 1) < 1e-5


# ---- the emulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("of", B.OFFSET_FIELDS)
@pytest.mark.parametrize("cid", [c.id for c in B.CASES])
def test_emulation_is_inside_the_bound(cid, of):
    vf = B.VALUE_FIELDS[(B.OFFSET_FIELDS.index(of) + [c.id for c in B.CASES].index(cid)) % 3]
    e, r = _emulate(cid, of, vf)
    ratios = B.check_all(e, r, f"{cid}/{of}/{vf}")
    print(cid, of, vf, ratios)
    assert max(ratios.values()) < 0.25      # sequential fp32 sums sit far below the ceiling; a mutant does not
    assert B.old_ok(e, r)


def test_emulation_modes():
    v, r = B.inputs("per2_straddle", "far", "noise")
    full, _ = _emulate("per2_straddle", "far", "noise")
    nodx, _ = _emulate("per2_straddle", "far", "noise", need_dx=False)
    assert nodx["dx"] is None
    for k in ("doff", "dmask", "dw"):
        assert np.array_equal(full[k].view(np.uint32), nodx[k].view(np.uint32)), k


# ---- mutants: (mutant, case, offset field, value field, the old metric accepts it) ------------------------------------------------
MUTANT_TABLE = (
    ("a", "per2_straddle", "converge", "masked", True),
    ("b", "per2_straddle", "seams", "masked", False),
    ("c", "per2_straddle", "far", "masked", False),
    ("d", "per2_straddle", "far", "masked", False),
    ("e", "per2_straddle", "noise", "masked", True),
    ("f", "per2_straddle", "noise", "masked", True),
    ("f1", "per2_straddle", "noise", "masked", False),
    ("f1", "per2_two_images", "noise", "blocks", False),
    ("g", "per2_straddle", "noise", "masked", True),
    ("e", "per3_splits", "noise", "masked", True),
    ("f", "per3_splits", "noise", "masked", True),
)


@pytest.mark.parametrize("mutant,cid,of,vf,old_accepts", MUTANT_TABLE, ids=lambda v: str(v))
def test_mutant_is_rejected_by_the_local_checks(mutant, cid, of, vf, old_accepts):
    e, r = _emulate(cid, of, vf, mutant=mutant)
    olds = {k: B.old_metric(e[k], ref) for k, ref, _ in r.pairs()}
    print(mutant, B.MUTANT_DOC[mutant], cid, of, vf, "old metric", olds)
    with pytest.raises(AssertionError, match="outside the local bound"):
        B.check_all(e, r, f"mutant {mutant}")
    assert B.old_ok(e, r) == old_accepts, olds


def test_mutants_of_the_window_are_invisible_without_the_inputs_that_reach_them():
    """what the old tests fed: sigma-noise offsets never reach window column 30 / 31, row 12 of wave 3 stays empty, multiplicities
    stay small -- mutants (a) and (b) are bit-identical to the emulation there, whatever the metric"""
    base, r = _emulate("per2_straddle", "noise", "noise")
    for mu in ("a", "b"):
        e, _ = _emulate("per2_straddle", "noise", "noise", mutant=mu)
        assert all(np.array_equal(e[k], base[k]) for k in ("dx", "doff", "dmask", "dw")), mu


def test_mutant_h_is_rejected_by_the_mode_comparison():
    full, r = _emulate("per1_ragged", "noise", "noise")
    e, _ = _emulate("per1_ragged", "noise", "noise", need_dx=False, mutant="h")
    assert np.array_equal(full["doff"], e["doff"]) and np.array_equal(full["dw"], e["dw"])
    assert not np.array_equal(full["dmask"], e["dmask"])
    with pytest.raises(AssertionError, match="outside the local bound"):
        B.check_all(e, r, "mutant h")
    assert set(B.MUTANTS) == {m[0] for m in MUTANT_TABLE} | {"h"} == set(B.MUTANT_DOC)
