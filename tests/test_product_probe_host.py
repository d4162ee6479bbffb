"""tests/product_probe.py on the CPU, all in float64: the split restatement is exact, the full emulation meets the bounds of
every probe class, every mutant (a kernel that loses a plane product somewhere) is rejected by the probes -- and the subtle ones are
NOT rejected by the metric the suite had before (2e-5 max|ref| on randn data), which is the gap the probes close."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import product_probe as P

N_PROBE = 1 << 14
LAYERS = ((3, 64, 64), (7, 8, 32), (7, 32, 64), (7, 16, 2), (5, 64, 120))


def _pairs(cls, n=N_PROBE, seed=1):
    return P.probe_pair(cls, n, n, seed)


def test_split_is_bit_exact_and_every_plane_is_bf16():
    rng = np.random.default_rng(0)
    pools = [np.concatenate(_pairs(c)) for c in P.CLASSES]
    u = rng.integers(0, 1 << 32, 1_000_000, dtype=np.uint64).astype(np.uint32)
    # finite patterns whose third plane is still a normal number (biased exponent >= 24; below, lo is a subnormal with more than
    # eight bits and the split is no longer three bf16 numbers -- 2^-103, far below anything the model holds), and the zeros
    u = u[(((u >> 23) & 0xFF) != 0xFF) & (((u >> 23) & 0xFF) >= 24)]
    u = np.concatenate([u, np.array([0, 0x80000000], np.uint32)])
    for x in pools + [P.floats(u)]:
        hi, mid, lo = P.split3(x)
        for plane in (hi, mid, lo):
            assert (P.bits(plane) & 0xFFFF == 0).all()      # bf16-representable
        total = (hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)).astype(np.float32)
        assert (hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64) == x.astype(np.float64)).all()
        assert (P.bits(total) == P.bits(x))[x != 0].all()   # bit for bit (x = -0: the planes sum to +0)
        # truncation: the planes carry x's sign and shrink by 2^-7 and 2^-15
        ax = np.abs(x.astype(np.float64))
        assert (np.abs(mid) < 2.0 ** -7 * ax)[ax >= 2.0 ** -100].all() and (np.abs(lo) < 2.0 ** -15 * ax)[ax >= 2.0 ** -100].all()
        assert (np.sign(mid) * np.sign(x) >= 0).all() and (np.sign(lo) * np.sign(x) >= 0).all()


def test_probe_classes_have_the_live_products_they_claim():
    for cls, (bx, bw) in P.CLASSES.items():
        x, w = _pairs(cls)
        assert P.is_normal(x) and P.is_normal(w) and P.is_normal(x.astype(np.float64) * w)
        e = np.floor(np.log2(np.abs(x.astype(np.float64))))
        assert e.min() >= -12 and e.max() <= 12
        px, pw = P.split3(x), P.split3(w)
        if cls != "D":
            for i in range(3):
                assert (px[i] != 0).all() == (8 * (i + 1) <= bx) and (px[i] == 0).all() == (8 * (i + 1) > bx), (cls, "x", i)
                assert (pw[i] != 0).all() == (8 * (i + 1) <= bw) and (pw[i] == 0).all() == (8 * (i + 1) > bw), (cls, "w", i)
            assert (P.emulate(x, w, P.DROPPED) == 0).all()                      # nothing a six-product kernel drops
            assert (P.emulate(x, w, P.LIVE[cls]) == x.astype(np.float64) * w).all()
            low = {"A": (0, 2), "B": (2, 0), "C": (1, 1)}[cls]
            assert (np.abs(P.emulate(x, w, [low])) >= 2.0 ** -17 * np.abs(x.astype(np.float64) * w) * (1 if cls != "C" else 0.5)).all()
        assert (P.emulate(x, w, P.ALL9) == x.astype(np.float64) * w).all()      # nine products: exact


def test_dropped_products_are_below_2_to_minus_21_not_2_to_minus_23():
    """the sources said "below 2^-23": each of mid*lo, lo*mid is below 2^-22, the three together below 2^-21, and operands exist
    next to that figure"""
    worst = 0.0
    for cls in ("D",):
        x, w = _pairs(cls, 1 << 18)
        rel = np.abs(P.emulate(x, w, P.DROPPED)) / np.abs(x.astype(np.float64) * w)
        assert (rel < P.DROP_REL).all()
        for p in ((1, 2), (2, 1)):
            assert (np.abs(P.emulate(x, w, [p])) < 2.0 ** -22 * np.abs(x.astype(np.float64) * w)).all()
        worst = max(worst, rel.max())
    # the extreme pair: first field smallest, the others all ones
    x = P.floats(np.array([0x3F80FFFF], np.uint32))
    rel = float(P.emulate(x, x, P.DROPPED)[0] / (float(x[0]) ** 2))
    assert 2.0 ** -21.1 < rel < 2.0 ** -21 and worst > 2.0 ** -22, (rel, worst)


@pytest.mark.parametrize("cls", list(P.CLASSES))
def test_the_full_emulation_meets_every_bound(cls):
    x, w = _pairs(cls)
    xw = x.astype(np.float64) * w
    for nprod in (6, 9):
        got = P.emulate(x, w, P.ALL9 if nprod == 9 else P.SIX)
        # the emulation has no accumulation error: it must sit inside the bound with the 16 u to spare
        assert (np.abs(got - xw) <= (P.one_product_bound(cls, nprod) - 16 * P.U) * np.abs(xw)).all(), (cls, nprod)
    assert P.one_product_bound("D", 9) == 16 * P.U and P.one_product_bound("A", 6) == 16 * P.U
    assert P.one_product_bound("D", 6) == 2.0 ** -21 + 16 * P.U and P.one_product_bound("C", 6, native=True) == 2 * P.U
    assert P.one_product_bound("D", 6, mask=True) == 2.0 ** -21 + 18 * P.U and P.one_product_bound("D", 6, native=True, mask=True) == 4 * P.U


def _schedule_elements(k, cin, cout, cls, seed=3):
    """one (x, w, tap) element per (channel, tap) pair of the layer, as the one-hot schedule pairs them"""
    sched = P.conv_schedule(k, cin, cout)
    tap = np.concatenate([t[t >= 0] for _, t in sched])
    x, w = P.probe_pair(cls, len(tap), len(tap), seed)
    return x, w, tap


def test_lo_times_lo_is_beyond_any_test_of_the_output():
    """the one single-product mutant no test rejects: lo*lo is below 2^-30 of the product, a 64th of an fp32 ulp of the output"""
    x, w = _pairs("D")
    assert (np.abs(P.emulate(x, w, [(2, 2)])) < 2.0 ** -30 * np.abs(x.astype(np.float64) * w)).all()


@pytest.mark.parametrize("name", [m for m in P.mutants() if m != "no_ll"])
def test_every_mutant_is_rejected(name):
    """a mutant exceeds the bound of at least one class by 8x somewhere on the schedule of every layer; the mutants whose loss is
    below the nine-product bound itself (BELOW_BOUND) fail the nine-minus-six criterion instead"""
    mut = P.mutants()[name]
    if name in P.BELOW_BOUND:
        x, w = _pairs("D")
        tap = np.zeros(len(x), int)
        out6 = P.emulate(x, w, P.SIX)
        got, want = P.nine_minus_six(P.emulate(x, w, P.ALL9), out6, x, w)
        assert got >= 0.75 * want > 0                                       # the honest nine-product run passes
        got, want = P.nine_minus_six(mut(x, w, tap, 3, 9), out6, x, w)
        assert got < 0.75 * want, (name, got, want)
        return
    for k, cin, cout in LAYERS:
        worst = 0.0
        for cls in P.CLASSES:
            x, w, tap = _schedule_elements(k, cin, cout, cls)
            xw = x.astype(np.float64) * w
            for nprod in (6, 9):
                rel = np.abs(mut(x, w, tap, k, nprod) - xw) / np.abs(xw)
                worst = max(worst, rel.max() / P.one_product_bound(cls, nprod))
        assert worst >= 8, (name, (k, cin, cout), worst)


def _plane_conv(x, w, mut_name, k):
    """float64 convolution as the mutant kernel would compute it (every output sums the mutant's products)"""
    mut = P.mutants()[mut_name]
    n, cin, h, wd = x.shape
    cols = F.unfold(torch.from_numpy(x), k, padding=k // 2).numpy().reshape(n, cin, k * k, h * wd)      # x per (ci, tap, pixel)
    tap = np.arange(k * k)[None, None, :, None]
    out = np.zeros((n, w.shape[0], h * wd))
    for co in range(w.shape[0]):
        wv = w[co].reshape(1, cin, k * k, 1)
        out[:, co] = mut(cols, np.broadcast_to(wv, cols.shape), np.broadcast_to(tap, cols.shape), k, 6).sum((1, 2))
    return out.reshape(n, -1, h, wd)


@pytest.mark.parametrize("k,cin,cout", [(3, 64, 64), (7, 8, 32)])
def test_the_previous_metric_does_not_see_the_subtle_mutants(k, cin, cout):
    """the gap: max|out - ref| <= 2e-5 max(1, max|ref|) on randn data, the comparison of tests/test_hip_ops.py and
    tests/test_hip_conv_routes.py, accepts a kernel that loses a low-order product; it does reject the gross mutants"""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, cin, 6, 9, generator=g).numpy()
    w = (torch.randn(min(cout, 8), cin, k, k, generator=g) * (cin * k * k) ** -0.5).numpy()
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), padding=k // 2).numpy()
    tol = 2e-5 * max(1.0, np.abs(ref).max())
    for name in P.SUBTLE:
        if name in ("no_ml", "no_lm", "no_ll", "nine_as_six"):
            continue                                        # six-product kernels never had them
        err = np.abs(_plane_conv(x, w, name, k) - ref).max()
        assert err <= tol, (name, err, tol)                 # accepted, although the product is lost at EVERY tap and channel
        assert err > 0
    for name in ("no_hm", "bf16_once", "rne_hi"):
        assert np.abs(_plane_conv(x, w, name, k) - ref).max() > tol, name


@pytest.mark.parametrize("k,cin,cout", LAYERS)
def test_conv_schedule_visits_every_pair_once(k, cin, cout):
    sched = P.conv_schedule(k, cin, cout)
    assert len(sched) == -(-cin * k * k // cout)
    seen = np.zeros((cin, k * k), int)
    for ci, tap in sched:
        assert len(ci) == cout and ((ci >= 0) == (tap >= 0)).all()
        np.add.at(seen, (ci[ci >= 0], tap[tap >= 0]), 1)
    assert (seen == 1).all()
    assert all(any((tap == t).any() for _, tap in sched) for t in P.last_pair_taps(k))      # the last tap pair is reached
    assert {(3, 64, 64): 9, (7, 32, 64): 25, (5, 64, 120): 14}.get((k, cin, cout), len(sched)) == len(sched)


def test_onehot_outputs_are_single_products():
    """the builders against a float64 convolution: every output is the one product (bit-exact in float64) or exactly zero"""
    k, cin, cout = 3, 16, 8
    x, _ = P.probe_pair("D", (2, cin, 9, 33), 1, 5)
    for j, (ci, tap) in enumerate(P.conv_schedule(k, cin, cout)[:4]):
        _, vals = P.probe_pair("D", 1, cout, 100 + j)
        wt = P.onehot_weight(k, cin, ci, tap, vals)
        xs, ws, inside = P.onehot_expected(x, k, ci, tap, vals)
        ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), padding=1).numpy()
        assert (ref == xs.astype(np.float64) * ws).all() and (np.count_nonzero(wt.reshape(cout, -1), axis=1) == 1).all()
        assert P.zeros_ok(ref, xs, ws, inside) and P.rel_error(ref, xs, ws, inside) == 0.0
        assert not inside[:, :, 0, 0].all() or (tap == 4).all()     # the image border holds padding zeros for the outer taps


@pytest.mark.parametrize("h,w", [(9, 36), (9, 33)])
def test_wgrad_schedule_visits_every_tile_position_once(h, w):
    pos = P.wgrad_positions(h, w)
    assert len(set(pos)) == len(pos) == 8 * 32 + 33 + 8
    assert {(y, x) for y in range(8) for x in range(32)} <= set(pos) and (8, 0) in pos and (8, 32) in pos and (0, 32) in pos
    sched = P.wgrad_schedule(h, w, 64)
    seen = [tuple(r[1:]) for a in sched for r in a if r[0] >= 0]
    assert sorted(seen) == sorted(pos) and len(sched) == 5
    # against a float64 weight gradient
    x, _ = P.probe_pair("D", (2, 8, h, w), 1, 7)
    _, vals = P.probe_pair("D", 1, 64, 8)
    dy = P.wgrad_onehot(2, h, w, sched[4], vals)
    xs, ws, inside = P.wgrad_expected(x, sched[4], vals)
    xd = torch.from_numpy(x).double()
    cols = F.unfold(xd, 3, padding=1).view(2, 8, 9, h * w)
    ref = torch.einsum("nop,nctp->oct", torch.from_numpy(dy).double().view(2, 64, -1), cols).view(64, 8, 3, 3).numpy()
    assert (ref == xs.astype(np.float64) * ws).all() and P.zeros_ok(ref, xs, ws, inside)


def test_nothing_is_subnormal_or_overflows():
    for cls in P.CLASSES:
        x, w = _pairs(cls)
        for planes in P.split3(x) + P.split3(w):
            assert P.is_normal(planes)
        for p in P.ALL9:
            assert P.is_normal(P.emulate(x, w, [p]).astype(np.float32))     # every plane product is a normal fp32 number or 0
    x, wt = P.dense_inputs(2, 64, 8, 9, 33, 3)
    assert P.is_normal(x) and P.is_normal(wt)
    S = F.conv2d(torch.from_numpy(x).double().abs(), torch.from_numpy(wt).double().abs(), padding=1)
    assert P.is_normal(S.numpy().astype(np.float32)) and S.max() < 2.0 ** 40
    e = np.log2(np.abs(x).reshape(2, 64, -1).max((0, 2)))
    assert e.min() < -15 and e.max() > 15                   # the scales are spread
