"""CPU proof of the fixtures in tests/h16_exact.py: the bit-exact GPU tests of the 16-bit kernels (tests/test_hip_h16_exact.py)
rest on inputs whose fp32 accumulation is exact in every order and on a target table that tells the right rounding from four
wrong ones.  Nothing here is assumed: every chunk, every product, every summation order, the fp32 against the fp64 convolution
and the four mutants are checked."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests import h16_exact as X

DTS = ("bf16", "fp16")
SHAPE = (2, 11, 37)
SOURCES = {"single": [(1, 0, 0), (1, 7, 31), (1, 10, 5), (1, 4, 36), (1, 3, 12)],
           "three": [(1, 0, 0), (1, 7, 31), (1, 8, 32), (1, 10, 5), (1, 4, 36), (1, 3, 12)]}
EPILOGUES = [("none", 0.0), ("relu", 0.0), ("lrelu", 0.125), ("lrelu", 0.25), ("res", 0.0)]
# what no convolution with normal 16-bit operands can produce (the conv builders leave them out; the elementwise kernels get them):
# fp16: one fp32 ulp beside 2^-25 (24 significant bits ending at 2^-48); bf16 behind LeakyReLU: -(range top) / slope overflows fp32
UNPLACED = {"fp16": 2, "bf16": 0}

_cache = {}


def cases(dt, flavour, epilogue, slope):
    key = (dt, flavour, epilogue, slope)
    if key not in _cache:
        _cache[key] = X.conv_cases(dt, SHAPE, SOURCES[flavour], flavour, epilogue, slope or 0.25)
    return _cache[key]


def representable(t, dt):
    return X.same_bits(t.to(X.DT[dt]).float(), t)


@pytest.mark.parametrize("dt", DTS)
def test_table_has_every_class_and_the_reference_rounding_is_torchs(dt):
    V, labels = X.targets(dt)
    assert set(labels) == set(X.CLASSES[dt])
    assert len(labels) == V.numel() and torch.isfinite(V).all()
    want = V.to(X.DT[dt])
    assert X.same_bits(X.round_to(V, dt, "rne"), want)          # the exact-arithmetic rounding below is the CPU's .to(dtype)
    lab = {c: torch.tensor([l_ == c for l_ in labels]) for c in X.CLASSES[dt]}
    # ties: halfway between two neighbours, both parities of the lower one, both signs, several exponents
    lo, hi = X.round_to(V, dt, "truncate").double(), X.round_to(V, dt, "away").double()
    t = lab["tie"]
    assert ((V.double()[t] - lo[t]) == (hi[t] - V.double()[t])).all() and (lo[t] != hi[t]).all()
    low_bits = X.bits_of(X.round_to(V, dt, "truncate"))[t] & 1
    assert set(low_bits.tolist()) == {0, 1} and (V[t] > 0).any() and (V[t] < 0).any()
    assert len(set(torch.frexp(V[t])[1].tolist())) >= 4
    # near-ties: one fp32 ulp beside a tie
    ties = set(X.bits_of(V)[t].tolist())
    assert all((b + 1 in ties) or (b - 1 in ties) for b in X.bits_of(V)[lab["near"]].tolist())
    # carries: the rounded value has a larger exponent than the target
    c = lab["carry"]
    assert (torch.frexp(want.float()[c])[1] == torch.frexp(V[c])[1] + 1).all()
    assert torch.equal(X.bits_of(V)[lab["zero"]], torch.tensor([0, -2 ** 31], dtype=torch.int32))
    top = want.float()[lab["top"]]
    assert torch.isinf(top).any() and (top.abs() == X.MAXF[dt]).any() and (top > 0).any() and (top < 0).any()
    if dt == "fp16":
        vals = set(V[lab["top"]].tolist())
        assert {65504.0, 65520.0, -65520.0, 131072.0} <= vals
        assert float(torch.nextafter(torch.tensor(65520.0), torch.tensor(0.0))) in vals
        s = want.float()[lab["subnormal"]]
        sv = set(V[lab["subnormal"]].tolist())
        assert {2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 1022.5 * 2.0 ** -24, 1023.5 * 2.0 ** -24} <= sv
        assert (s.abs() <= 2.0 ** -14).all() and (s == 0).any() and (s.abs() == 2.0 ** -14).any()
        assert V.to(torch.float16)[labels.index("subnormal")].item() == 0.0           # 2^-25 -> 0 (tie to even)
        assert torch.tensor(3 * 2.0 ** -25).to(torch.float16).item() == 2.0 ** -23


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("how,classes", [("truncate", ("tie", "near", "carry")), ("away", ("tie",)), ("flush", ("subnormal",)),
                                         ("clamp", ("top",))])
def test_each_wrong_rounding_is_caught_by_the_classes_meant_for_it(dt, how, classes):
    """the check that the table can fail: a kernel that truncates, rounds ties away from zero, flushes subnormal results or
    saturates at the largest finite value differs from V.to(dtype) on at least one entry of EVERY class meant to catch it"""
    if how == "flush" and dt == "bf16":
        return                      # (the table holds no bf16 subnormal: no convolution here could produce one exactly)
    V, labels = X.targets(dt)
    want, got = V.to(X.DT[dt]), X.round_to(V, dt, how)
    diff = X.bits_of(want) != X.bits_of(got)
    for c in classes:
        m = torch.tensor([l_ == c for l_ in labels])
        assert diff[m].any(), (how, c)
    # and the mutant is no strawman: it agrees with the right rounding on most of the table
    assert (~diff).sum() >= V.numel() // 3


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("flavour", ["single", "three"])
@pytest.mark.parametrize("epilogue,slope", EPILOGUES)
def test_conv_cases_are_exact_in_every_order(dt, flavour, epilogue, slope):
    V, labels = X.targets(dt)
    cs = cases(dt, flavour, epilogue, slope)
    seen = set()
    for c in cs:
        # operands: representable in the 16-bit type, and normal (or zero)
        for t in (c.x, c.weight) + ((c.skip,) if c.skip is not None else ()):
            assert representable(t, dt)
        nz = torch.cat([c.x[c.x != 0].abs(), c.weight[c.weight != 0].abs()])
        assert (nz >= 2.0 ** X.EMIN[dt]).all() and (nz <= X.MAXF[dt]).all()
        assert not torch.signbit(c.weight[c.weight == 0]).any()          # no -0 weight: an untouched pixel sums to +0
        for pl in c.placed:
            seen.add(pl.index)
            ch = torch.tensor(pl.chunks + (pl.s,), dtype=torch.float64)
            assert X.same_bits(ch.to(X.DT[dt]).double(), ch)             # to the 16-bit type and back: the identity
            prods = [torch.tensor(cj, dtype=torch.float32) * torch.tensor(pl.s, dtype=torch.float32) for cj in pl.chunks]
            assert all(float(p_) == cj * pl.s for p_, cj in zip(prods, pl.chunks))       # the products are exact
            assert all(cj == 0 or (cj > 0) == (pl.a > 0) for cj in pl.chunks)
            for order in itertools.permutations(range(3)):               # all six summation orders in fp32
                acc = torch.tensor(0.0, dtype=torch.float32)
                for j in order:
                    acc = acc + prods[j]
                assert float(acc) == pl.a, (pl, order)
                # ... and starting from the bias (a kernel may initialise its accumulator with it)
                acc = c.bias[pl.co].clone()
                for j in order:
                    acc = acc + prods[j]
                assert float(acc) == pl.pre, (pl, order)
            assert float(torch.tensor(pl.a, dtype=torch.float32) + c.bias[pl.co]) == pl.pre
        # the convolution in fp32 and in fp64 agree bit for bit at every pixel, the untouched ones included
        a32 = F.conv2d(c.x, c.weight, None, 1, 1)
        a64 = F.conv2d(c.x.double(), c.weight.double(), None, 1, 1)
        assert X.same_bits(a32, a64.float()) and torch.equal(a64, a64.float().double()) and X.same_bits(a32, c.acc)
        p32 = F.conv2d(c.x, c.weight, c.bias, 1, 1)
        assert X.same_bits(p32, c.pre) and torch.equal(c.pre.double(), a64 + c.bias.double().view(1, -1, 1, 1))
        # the epilogue is exact in fp32
        n = c.x.shape[0]
        if epilogue == "relu":
            w64, w32 = torch.relu(c.pre.double()), torch.relu(c.pre)
        elif epilogue == "lrelu":
            w64, w32 = F.leaky_relu(c.pre.double(), slope), torch.maximum(c.pre, c.pre * slope)
        elif epilogue == "res":
            w64 = c.skip.double() + c.scale.double().view(n, -1, 1, 1) * c.pre.double()
            w32 = c.skip + c.scale.view(n, -1, 1, 1) * c.pre
            assert (torch.log2(c.scale) == torch.log2(c.scale).round()).all()
        else:
            w64, w32 = c.pre.double(), c.pre
        assert torch.equal(w64, c.want32.double()) and X.same_bits(w32, c.want32)
        assert (torch.log2(c.bias.abs()) == torch.log2(c.bias.abs()).round()).all()      # dyadic bias
        # the targets land where `hit` says, and everything else is the epilogue of the bias alone
        assert X.same_bits(X.final_values(c, V), c.want32)
        free = (c.acc == 0)
        assert (c.hit[free] == -1).all() and free.sum() > free.numel() // 2
        if flavour == "single":
            assert (c.hit[~free] >= 0).all()         # (in the three-tap flavour a stamp cut by the image edge leaves a partial sum)
        assert not torch.signbit(c.acc[free]).any()
    shown = set()
    for c in cs:
        shown |= set(c.hit[c.hit >= 0].tolist())
    lost = V.numel() - len(seen)
    if epilogue == "lrelu" and dt == "bf16":
        assert lost == 5 and all(labels[i] == "top" and V[i] < 0 for i in range(V.numel()) if i not in seen)
    else:
        assert lost == UNPLACED[dt], lost
    assert shown == seen                              # every placed target is visible at some pixel of this shape
    for cl in X.CLASSES[dt]:
        assert any(labels[i] == cl for i in shown), cl


@pytest.mark.parametrize("dt", DTS)
def test_three_tap_flavour_keeps_the_chunks_in_three_taps_and_single_in_one_block(dt):
    for c in cases(dt, "three", "none", 0.0):
        for pl in c.placed:
            taps = [tuple(i.tolist()) for i in (c.weight[pl.co, list(pl.channels)] != 0).nonzero()]
            assert all(t_[1] == 1 and t_[2] == t_[0] for t_ in taps)     # chunk j at tap (1, j)
    for c in cases(dt, "single", "none", 0.0):
        for pl in c.placed:
            assert len({ch // 16 for ch in pl.channels}) == 1             # one k-step of the 16-bit MFMA
            assert (c.weight[pl.co, list(pl.channels), pl.tap[0], pl.tap[1]] == torch.tensor(pl.chunks)).all()
    assert len({pl.tap for c in cases(dt, "single", "none", 0.0) for pl in c.placed}) >= 3


@pytest.mark.parametrize("dt", DTS)
def test_other_convolution_shapes(dt):
    """the builders at the shapes the GPU tests use for the other kernels: 3 output channels, 5 x 5, 256 output channels,
    degenerate images"""
    V, _ = X.targets(dt)
    for kw in (dict(cout=3), dict(cout=72, ksize=5), dict(cout=256)):
        k = kw.get("ksize", 3)
        cs = X.conv_cases(dt, (1, 8, 32), [(0, 0, 0), (0, 7, 31), (0, 3, 16)], "single", "none", **kw)
        for c in cs:
            a32 = F.conv2d(c.x, c.weight, c.bias, 1, k // 2)
            a64 = F.conv2d(c.x.double(), c.weight.double(), c.bias.double(), 1, k // 2)
            assert X.same_bits(a32, a64.float()) and X.same_bits(a32, c.want32) and X.same_bits(X.final_values(c, V), c.want32)
    for shape, src in (((1, 1, 1), [(0, 0, 0)]), ((1, 1, 40), [(0, 0, 0), (0, 0, 33)]), ((1, 33, 1), [(0, 0, 0), (0, 32, 0)])):
        for fl in ("single", "three"):
            for c in X.conv_cases(dt, shape, src, fl, "relu"):
                a32 = torch.relu(F.conv2d(c.x, c.weight, c.bias, 1, 1))
                assert X.same_bits(a32, c.want32)


@pytest.mark.parametrize("dt", DTS)
def test_scale_residual_case_is_exact_and_shows_the_whole_table(dt):
    V, labels = X.targets(dt)
    shown = set()
    for page in range(2):
        r, scale, x, want, idx = X.scale_residual_case(dt, 2, 3, 5, page=page)
        assert representable(r, dt) and representable(x, dt)
        w64 = r.double() * scale.double().view(2, 64, 1, 1) + x.double()
        assert torch.equal(w64, want.double())
        assert X.same_bits(r * scale.view(2, 64, 1, 1) + x, want)
        one = (r == 1.0)
        assert X.same_bits(want[one], (V[idx] + 0.0).view(2, 64, 1, 1).expand_as(want)[one])      # (-0 - (-0) + (-0) = +0)
        shown |= set(idx.tolist())
    assert shown == set(range(V.numel()))


def test_same_bits_treats_nan_as_nan_and_signed_zero_as_different():
    a = torch.tensor([1.0, float("nan"), 0.0])
    assert X.same_bits(a, torch.tensor([1.0, float("nan"), 0.0]))
    assert not X.same_bits(a, torch.tensor([1.0, float("nan"), -0.0]))
    assert not X.same_bits(a, torch.tensor([1.0, 2.0, 0.0]))
    assert "differ" in X.mismatches(a, torch.tensor([1.0, 2.0, 0.0]))
