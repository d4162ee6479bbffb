"""Host side of the Winograd kernel's contract (tests/wino4_contract.py): the numpy restatement agrees with torch in
double, the fp32 emulation -- the stand-in for a correct kernel -- meets the per-pixel bound on every case and fixes K, each
mutant is rejected by the new checks (and what the checks of tests/test_hip_ops.py say about it), the case table covers what it
claims to.  No GPU, no library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wino4_contract as W


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).double()


def _torch_ref(c, x, p):
    y = F.conv2d(_t(x), _t(p["w"]), _t(p["bias"]), 1, c.k // 2)
    y = F.relu(y) if c.act == "relu" else F.leaky_relu(y, float(W.SLOPE)) if c.act == "lrelu" else y
    if p["res_scale"] is not None:
        y = y * _t(p["res_scale"])[:, :, None, None]
    if p["residual"] is not None:
        y = y + _t(p["residual"])
    return (F.pixel_shuffle(y, 2) if c.shuffle else y).numpy()


# ------------------------------------------------------------------------------------------ agreement with the references
@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.id)
def test_ref64_is_torch_conv2d_in_double_and_the_matrices_are_a_convolution(c):
    p = c.params()
    x, xx, cv, _ = c.operands("noise", p)
    if c.ca:
        x = (_t(x) * _t(p["ca_scale"])[:, :, None, None] + _t(xx)).numpy()
    plain = F.conv2d(_t(x), _t(p["w"]), None, 1, c.k // 2).numpy()
    scale = np.abs(plain).max()
    assert np.abs(cv.conv - plain).max() <= 1e-13 * scale
    assert np.abs(cv.epilogue(**c.epilogue_args(p)).ref - _torch_ref(c, x, p)).max() <= 1e-13 * max(1.0, scale)
    # B^T, G, A^T and the tile geometry, evaluated in fp64: this IS the convolution (the independent check of the weight pack's formula)
    assert np.abs(W.winograd64(x, p["w"]) - plain).max() <= 1e-12 * scale
    assert (cv.E >= np.abs(cv.conv) * (1 - 1e-12)).all()


def test_act_follows_eavsr_act_for_non_finite_values():
    v = np.array([np.nan, -np.inf, np.inf, -2.0, -0.0, 0.0, 3.0], np.float32)
    r = W.act_of(v, "relu")
    assert np.isnan(r[0]) and r[2] == np.inf and (r[[1, 3, 4, 5]] == 0).all() and not np.signbit(r[[1, 3, 4, 5]]).any() and r[6] == 3
    l = W.act_of(v, "lrelu")
    assert np.isnan(l[0]) and l[1] == -np.inf and l[2] == np.inf and l[3] == np.float32(-2.0) * W.SLOPE
    assert np.array_equal(W.act_of(v, None), v, equal_nan=True)


_ratios = {}


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.id)
def test_emulation_meets_the_bound_on_every_case(c):
    p = c.params()
    worst = 0.0
    for kind in W.INPUT_KINDS:
        _, _, cv, x = c.operands(kind, p)
        ratio = W.ratio_uE(W.emulate32(x, p["w"]), cv.conv, cv.E)
        r = cv.epilogue(**c.epilogue_args(p))
        out, pre = W.emulate32(x, p["w"], **c.epilogue_args(p), want_pre=True)
        rel = W.check_local(out, r, what=f"{c.id}/{kind}")
        old = W.old_global(out, r.ref)
        print(f"{c.id}/{kind}: emulation err/(u E) {ratio:.4f}  err/bound {rel:.3f}  old metric {old:.2e}")
        assert old <= W.OLD_GLOBAL_TOL
        worst = max(worst, ratio)
        if c.part:
            part, data, pr, pc = W.emulate_sums(pre, c.k)
            W.check_part(part, r, c.k, c.id)
            if c.border:
                W.check_pieces(data, pr, pc, r, c.id)
    _ratios[c.id] = worst


def test_K_is_four_times_the_emulation_and_under_the_rigorous_ceiling():
    """K is not chosen: 4 x the largest err / (u E) of emulate32 over the table's own inputs (the factor: the kernel's other, equally
    legitimate association order).  The ceiling it may never pass is the worst case (cin + C0) u E of the smallest cin."""
    missing = [c for c in W.CASES if c.id not in _ratios]
    for c in missing:      # (run alone: compute what the parametrised test would have left)
        test_emulation_meets_the_bound_on_every_case(c)
    worst = max(_ratios.values())
    print("largest emulation ratio", repr(worst), "K", W.K)
    assert abs(W.K_EMULATION_RATIO - worst) <= 1e-3 * worst, (W.K_EMULATION_RATIO, worst)
    assert W.K == W.K_FACTOR * W.K_EMULATION_RATIO and W.K_FACTOR == 4.0
    assert W.K <= min(c.cin for c in W.CASES) + W.C0


# ------------------------------------------------------------------------------------------ mutants
def _rejects(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _local_verdicts(c, x, mutant):
    p = c.params()
    r = W.Conv(x, p["w"]).epilogue(**c.epilogue_args(p))
    good = W.emulate32(x, p["w"], **c.epilogue_args(p))
    W.check_local(good, r, what="emulate32")                   # the check accepts the correct emulation on this very input
    assert W.old_global(good, r.ref) <= W.OLD_GLOBAL_TOL
    bad = W.emulate32(x, p["w"], **c.epilogue_args(p), mutant=mutant)
    return _rejects(lambda: W.check_local(bad, r, what=mutant)), W.old_global(bad, r.ref) > W.OLD_GLOBAL_TOL


# mutant -> (case, input, does the OLD check (6e-5 max) reject it too?)
LOCAL_MUTANTS = {
    # (on white noise this one reaches only 0.48 of the bound K = 13.4 allows -- and 4.2e-5 on the old metric: accepted by both;
    # the frame of mixed dynamic range is where the per-pixel bound is tight enough: 3.1 x the bound, old metric 5.2e-5)
    "bt_lowbit": ("h8_w64", "blocks_on", False),
    "leak": ("rounds", "blocks_on", False),
    "leak_rows": ("seams_h40_w68", "blocks_on", False),
    "clamp_halo": ("h12_w124", "quiet_edge", False),
    # rounding the patch to bf16 is an error of 2^-9 per input: the old check sees it as well.  Not an argument for the new check
    # -- kept as the one mutant BOTH must reject, so that the table says what the old check is good for.
    "bf16_patch": ("h8_w64", "noise", True),
}


@pytest.mark.parametrize("mutant", sorted(LOCAL_MUTANTS))
def test_local_bound_rejects_the_mutant_and_what_the_old_metric_says(mutant):
    cid, kind, old_rejects = LOCAL_MUTANTS[mutant]
    c = W.case(cid)
    x = c.x(kind)
    new, old = _local_verdicts(c, x, mutant)
    assert new, f"the per-pixel bound accepts {mutant}"
    assert old == old_rejects, f"old metric on {mutant}: rejects = {old}"


def test_impulse_locality_rejects_the_leak_and_the_old_metric_accepts_it():
    ic = next(i for i in W.IMPULSES if i.id == "rounds")
    x, w = ic.x(), ic.weight()
    r = W.Conv(x, w).epilogue()
    zeros = W.check_impulse(W.emulate32(x, w), x, r, ic.k, "emulate32")
    assert zeros > 0.9 * x.shape[0] * ic.cout * ic.h * ic.w
    bad = W.emulate32(x, w, mutant="leak")
    assert _rejects(lambda: W.check_impulse(bad, x, r, ic.k, "leak"))
    assert W.old_global(bad, r.ref) <= W.OLD_GLOBAL_TOL


def test_non_finite_containment_rejects_nan_made_zero_and_the_old_checks_never_see_it():
    n, cin, h, wd = W.NONFINITE_SHAPE
    c = W._c("nf", n, h, wd, [cin], 8)
    p = c.params()
    for val in (np.inf, np.nan):
        for (y, x_) in W.NONFINITE_PIXELS:
            x = c.x("noise")
            x0 = x.copy()
            x0[1, 3, y, x_] = 0
            x[1, 3, y, x_] = val
            r0 = W.Conv(x0, p["w"]).epilogue(bias=p["bias"])
            cnt = W.check_nonfinite(W.emulate32(x, p["w"], bias=p["bias"]), (1, 3, y, x_), p["w"], r0, 3, "emulate32")
            assert cnt >= 4 * 8          # at least the receptive field of a corner pixel, every channel
            if np.isnan(val):
                bad = W.emulate32(x, p["w"], bias=p["bias"], mutant="nan_zero")
                assert _rejects(lambda: W.check_nonfinite(bad, (1, 3, y, x_), p["w"], r0, 3, "nan_zero"))
    # on finite data (all the old checks ever feed) the mutant IS the emulation, bit for bit: no old check can reject it
    x = c.x("noise")
    assert np.array_equal(W.emulate32(x, p["w"], mutant="nan_zero"), W.emulate32(x, p["w"]))


@pytest.mark.parametrize("mutant", W.SUM_MUTANTS)
def test_exchanged_slots_are_rejected_slot_by_slot_and_accepted_after_summing(mutant):
    c = W.case("h15_w64")
    x, p = c.x("noise"), c.params()
    r = W.Conv(x, p["w"]).epilogue(**c.epilogue_args(p))
    _, pre = W.emulate32(x, p["w"], **c.epilogue_args(p), want_pre=True)
    part, data, pr, pc = W.emulate_sums(pre, c.k)
    W.check_part(part, r, c.k)
    W.check_pieces(data, pr, pc, r)
    mpart, mdata, _, _ = W.emulate_sums(pre, c.k, mutant)
    if mutant == "swap_part":
        assert _rejects(lambda: W.check_part(mpart, r, c.k))
        assert W.old_part_ok(mpart, r.pre)                       # the sum over the tile axis does not move
    else:
        assert _rejects(lambda: W.check_pieces(mdata, pr, pc, r))
        assert np.allclose(mdata.sum(axis=2), data.sum(axis=2), rtol=1e-6, atol=0)      # nor does the sum over the pieces


# ------------------------------------------------------------------------------------------ the packed form's restatement
def test_unpack_inverts_the_documented_layout():
    cout, cin = 70, 8
    u = np.arange(128 * cin * 36, dtype=np.float64).reshape(128, cin, 6, 6)
    packed = np.empty((2, cin // 4, 18, 4, 64, 2))
    for pair in range(18):
        for lo in range(2):
            i, q = W.slot_position(pair, lo)
            for c in range(4):
                for col in range(64):
                    packed[:, :, pair, c, col, lo] = u.reshape(2, 64, cin // 4, 4, 6, 6)[:, col ^ (16 * (c & 1)), :, c, i, q]
    assert np.array_equal(W.unpack_u(packed.ravel(), cout, cin), u)
    assert sorted(W.slot_position(p, l) for p in range(18) for l in range(2)) == [(i, q) for i in range(6) for q in range(6)]


def test_multiples_of_576_pack_exactly():
    r = np.random.default_rng(1)
    for k in (3, 5):
        m = r.integers(-8, 9, (3, 4, k, k))
        exact = W.pack_exact(m)
        assert np.abs(exact).max() < 2 ** 24                                        # an fp32 holds it
        # the evaluation in double (1/6 is not a double) rounds ONCE to the exact value: what the pack kernel must return, bit for bit
        W.check_pack(W.pack_u64((576 * m).astype(np.float32)).astype(np.float32), m)
        hot = np.zeros_like(m)
        hot[2, 1, k - 1, 1] = 5
        u = W.pack_u64((576 * hot).astype(np.float32)).astype(np.float32)
        assert np.array_equal(u, W.pack_exact(hot).astype(np.float32)) and (u[2, 1] != 0).sum() >= 16 and (u != 0).sum() == (u[2, 1] != 0).sum()
        wrong = u.copy()
        wrong[2, 1, 3, 4] = np.nextafter(wrong[2, 1, 3, 4], np.float32(np.inf))
        with pytest.raises(AssertionError):
            W.check_pack(wrong, hot)


# ------------------------------------------------------------------------------------------ coverage of the case table
def test_case_table_covers_what_it_claims():
    three = [c for c in W.CASES if c.k == 3]
    assert {c.h % 8 for c in three} == set(range(8))
    assert {0, 4, 60} <= {c.w % 64 for c in three} and any(c.w < 64 for c in three)
    assert {7, 40, 64, 130} <= {c.cout for c in three} and any(-(-c.cout // 64) == 3 for c in three)
    assert any(c.wg_tiles > 256 for c in three) and any(i.n * 2 * 1 > 256 for i in W.IMPULSES if i.id == "rounds")
    chunks = {(c.cin // 4) % 2 for c in three}
    assert chunks == {0, 1}
    assert all(c.via == "cabi" for c in three if (c.cin // 4) % 2) and all(c.w % 4 == 0 for c in W.CASES)
    assert any(c.k == 5 and len(c.couts) == 3 for c in W.CASES)
    assert any(c.part and c.h % 8 == 1 for c in three) and any(c.part and c.w % 64 for c in three)      # a single valid row; ragged right
    assert any(c.border and c.w > 128 for c in three) and any(c.border and c.w <= 64 for c in three)
    assert len({c.id for c in W.CASES}) == len(W.CASES)
    # the dynamic-range frames have seams in BOTH directions, on the grids and one pixel off them
    for k, m, toh, tow in ((3, 4, 8, 64), (5, 2, 4, 32)):
        on = [c.seams("blocks_on") for c in W.CASES if c.k == k]
        off = [c.seams("blocks_off") for c in W.CASES if c.k == k]
        assert any(y % toh == 0 for r, _ in on for y in r), k                        # a row seam between two workgroup tiles
        assert k == 5 or any(y % m == 0 and y % toh for r, _ in on for y in r)      # and one between the two tile rows of a workgroup (12 = 4 mod 8;
                                                                                    # every multiple of 12 is one of 4: F(2x2,5x5) has none)
        assert any(x % tow == 0 for _, q in on for x in q) and any(x % m == 0 and x % tow for _, q in on for x in q), k
        assert any(y % m for r, _ in off for y in r) and any(x % m for _, q in off for x in q), k
    assert any(c.border and c.residual for c in W.CASES) and any(c.ca for c in W.CASES)
    assert set(W.INPUT_KINDS) >= {"noise", "offset100", "blocks_on", "blocks_off", "quiet_edge"}


@pytest.mark.parametrize("ic", [i for i in W.IMPULSES if i.images is None], ids=lambda i: i.id)
def test_impulses_take_all_36_patch_positions_at_corner_edge_and_interior_tiles(ic):
    seen = W.impulse_positions(ic)
    every = {(i, j) for i in range(6) for j in range(6)}
    for place in ("corner", "edge", "interior"):
        assert seen[place] == every, (place, sorted(every - seen[place]))
