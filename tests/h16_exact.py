"""Inputs for which a 16-bit kernel has exactly ONE right answer (plain torch on the CPU; nothing here imports the GPU package).

A tolerance of one 16-bit ulp of the largest element cannot tell round-to-nearest-even from truncation, from ties-away, from a
flushed subnormal or from a clamp at the largest finite value.  So the tests of the 16-bit kernels are given inputs whose fp32
accumulator is EXACT -- every product and every partial sum, in any order, is representable in fp32 -- and whose exact value
sits where the roundings differ: on a tie, one fp32 ulp beside a tie, under a carry, at the top of the range, among the
subnormals.  The 16-bit output then has one right answer, `V.to(dtype)` on the CPU, and is compared bit for bit.

* `targets(dt)`: the table of fp32 target values with their classes.
* `conv_cases(dt, ...)`: convolutions (input, weights, bias, skip, scale) that put the table's values into chosen pixels.  The
  input is zero except for a power of two `s` in three input channels of a source pixel; the weights of an output channel hold
  three chunks of A / s, where A = (value in front of the epilogue) - bias and the chunks are DISJOINT RANGES OF A's MANTISSA
  BITS (same sign, no overlap), so that every partial sum is a subset of A's bits.  (A three-way round-to-nearest split also
  sums back exactly, but not in every order for bf16, and for fp16 its third term often falls below the normal range.)  `s` is
  chosen so that `s` and every chunk are normal numbers of the 16-bit type.  Flavour "single": the three chunks sit in ONE tap
  (three input channels of one 16-channel block: they meet inside one k-step of the matrix pipe).  Flavour "three": they sit in
  three taps of the centre row and meet only in the accumulator.
* `round_to(v, dt, how)`: round-to-nearest-even and four wrong roundings in exact float64 arithmetic, for the host test that
  proves that the table can fail.

`tests/test_h16_exact_host.py` proves every claim made here on the CPU; the builders assume nothing.
"""
from __future__ import annotations

import math
import struct
from fractions import Fraction
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"bf16": 7, "fp16": 10}              # stored mantissa bits
EMIN = {"bf16": -126, "fp16": -14}          # exponent of the smallest normal number
EMAX = {"bf16": 127, "fp16": 15}            # exponent of the largest finite number
MAXF = {"bf16": float.fromhex("0x1.fep127"), "fp16": 65504.0}
CLASSES = {"bf16": ("tie", "near", "carry", "zero", "top"), "fp16": ("tie", "near", "carry", "zero", "top", "subnormal")}
SLOPES = (0.125, 0.25)


def f32_from_bits(bits: Sequence[int]) -> torch.Tensor:
    return torch.from_numpy(np.array(list(bits), dtype=np.uint32).view(np.float32).copy())


def bits_of(t: torch.Tensor) -> torch.Tensor:
    """the raw words of a tensor (int64 for fp64, int32 for fp32, int16 for the 16-bit types)"""
    return t.contiguous().view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, torch.int16))


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """bit for bit, except that a NaN matches any NaN"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    gn, wn = torch.isnan(got), torch.isnan(want)
    if not torch.equal(gn, wn):
        return False
    return torch.equal(bits_of(got)[~gn], bits_of(want)[~wn])


def mismatches(got: torch.Tensor, want: torch.Tensor, limit: int = 8) -> str:
    """the first few positions at which same_bits fails (for an assertion's message)"""
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    gn, wn = torch.isnan(got), torch.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (bits_of(got) != bits_of(want)))
    idx = bad.nonzero()
    rows = [f"{tuple(i.tolist())}: got {got[tuple(i)].item()!r} want {want[tuple(i)].item()!r}" for i in idx[:limit]]
    return f"{int(bad.sum())} of {bad.numel()} differ: " + "; ".join(rows)


# ---------------------------------------------------------------------------------------------------------------------------
# the target table
# ---------------------------------------------------------------------------------------------------------------------------
def targets(dt: str) -> Tuple[torch.Tensor, List[str]]:
    """(V, labels): fp32 values and the class of each (CLASSES[dt]).  The right 16-bit answer of every entry is V.to(DT[dt])."""
    p = MANT[dt]
    sh = 23 - p                     # fp32 mantissa bits below the 16-bit type's last one
    half = 1 << (sh - 1)            # the tie bit
    full = (1 << p) - 1
    bits: List[int] = []
    labels: List[str] = []

    def add(label, b):
        bits.append(b & 0xFFFFFFFF)
        labels.append(label)

    # (fp16: not below 2^-4 -- the last of a target's 24 bits, divided by a normal fp16 `s`, must itself be a normal fp16 number)
    exps = (-9, -1, 0, 6, 20) if dt == "bf16" else (-4, -1, 0, 6, 14)
    mids = (0, 1, 2, 0b0101010, 0b0101011, full - 1) if dt == "bf16" else (0, 1, 2, 0b0101010101, 0b1101010110, full - 1)
    for sign in (0, 1):
        for e in exps:
            base = (sign << 31) | ((e + 127) << 23)
            for m in mids:          # both parities of the lower neighbour
                t = base | (m << sh) | half
                add("tie", t)
                add("near", t + 1)
                add("near", t - 1)
            add("carry", base | 0x7FFFFF)                   # a mantissa of all ones: rounds up into the next exponent
            add("carry", base | (full << sh) | half)        # a tie under an odd all-ones neighbour: to even = a carry
            add("carry", base | (full << sh) | half | 1)
    add("zero", 0x00000000)
    add("zero", 0x80000000)
    if dt == "fp16":
        b65520 = struct.unpack("<I", struct.pack("<f", 65520.0))[0]
        for v in (65504.0, 65520.0, -65520.0, 65536.0, 65536.0 + 32.0, 100000.0, 131072.0, -131072.0, -65504.0):
            add("top", struct.unpack("<I", struct.pack("<f", v))[0])
        add("top", b65520 - 1)                              # 65519.996..: the last value that rounds to 65504
        add("top", (b65520 - 1) | 0x80000000)
        add("top", b65520 + 1)
        u = 2.0 ** -24                                      # the subnormal step
        subs = [0.5 * u, 1.5 * u, u, 0.25 * u, -0.5 * u, -1.5 * u, 0.75 * u]
        subs += [(m + 0.5) * u for m in (1, 2, 5, 6, 511, 512, 1021)]          # ties inside the subnormal range
        subs += [1022.5 * u, 1023.5 * u, -1022.5 * u, -1023.5 * u, 1023.0 * u, 3.0 * u]      # the largest subnormal -+ half a step
        for v in subs:
            add("subnormal", struct.unpack("<I", struct.pack("<f", v))[0])
        bh = struct.unpack("<I", struct.pack("<f", 0.5 * u))[0]
        add("subnormal", bh + 1)                            # one fp32 ulp above the tie with zero: rounds to the first subnormal
        add("subnormal", bh - 1)
    else:
        for b in (0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF):     # the largest bf16 | just below | at | above the boundary | fp32 max
            add("top", b)
            add("top", b | 0x80000000)
    return f32_from_bits(bits), labels


# ---------------------------------------------------------------------------------------------------------------------------
# roundings in exact arithmetic (float64 holds every quantity involved exactly)
# ---------------------------------------------------------------------------------------------------------------------------
def round_to(v: torch.Tensor, dt: str, how: str = "rne") -> torch.Tensor:
    """fp32 -> 16-bit type.  how: "rne" (the right one) | "truncate" | "away" (ties away from zero) | "flush" (round to nearest
    even, subnormal results to zero) | "clamp" (round to nearest even, saturate at the largest finite value)"""
    p, emin, maxf = MANT[dt], EMIN[dt], MAXF[dt]
    out = []
    for x in v.double().tolist():
        if x == 0.0 or math.isinf(x) or math.isnan(x):
            out.append(x)
            continue
        a = abs(x)
        e = max(math.frexp(a)[1] - 1, emin)
        step = 2.0 ** (e - p)
        q = a / step                                    # exact: a power-of-two scaling
        fl = math.floor(q)
        fr = q - fl
        if how == "truncate":
            n = fl
        elif how == "away":
            n = fl + (1 if fr >= 0.5 else 0)
        else:
            n = fl + (1 if fr > 0.5 or (fr == 0.5 and fl % 2 == 1) else 0)
        r = n * step
        if r > maxf:
            r = maxf if how == "clamp" else (maxf if how == "truncate" else math.inf)
        if how == "flush" and r < 2.0 ** emin:
            r = 0.0
        out.append(math.copysign(r, x))
    return torch.tensor(out, dtype=torch.float64).to(DT[dt])


# ---------------------------------------------------------------------------------------------------------------------------
# exact convolutions
# ---------------------------------------------------------------------------------------------------------------------------
def _exact32(x: float) -> bool:
    if math.isinf(x) or math.isnan(x):
        return False
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0] == x
    except OverflowError:
        return False


def _exp_of(x: float) -> int:
    return math.frexp(abs(x))[1] - 1


def _pow2_in(dt: str, e: int) -> float:
    return 2.0 ** min(max(e, EMIN[dt]), EMAX[dt])


def split3(a: float) -> Tuple[float, float, float]:
    """an fp32 value as three same-signed pieces holding mantissa bits 23..16, 15..8 and 7..0 (+0 where a range is empty)"""
    if a == 0.0:
        return (0.0, 0.0, 0.0)
    b = struct.unpack("<I", struct.pack("<f", a))[0]
    ex = (b >> 23) & 0xFF
    assert 0 < ex < 255, "split3: a normal fp32 number expected"
    mant = (b & 0x7FFFFF) | 0x800000
    unit = math.ldexp(1.0, ex - 127 - 23)
    sg = -1.0 if b >> 31 else 1.0
    return tuple((sg * ((mant & m) * unit)) if (mant & m) else 0.0 for m in (0xFF0000, 0x00FF00, 0x0000FF))


def _scale_for(dt: str, chunks: Sequence[float], have: Sequence[int]) -> Optional[int]:
    """k with s = 2^k such that s and every non-zero chunk / s are normal numbers of the type; prefers a k already in use"""
    nz = [abs(c) for c in chunks if c != 0.0]
    lo, hi = EMIN[dt], EMAX[dt]
    if nz:
        # a chunk has at most 8 significant bits: it is representable as soon as its leading bit is in the normal range
        hi = min(hi, min(_exp_of(c) for c in nz) - EMIN[dt])
        lo = max(lo, max(_exp_of(c) for c in nz) - EMAX[dt])
    if lo > hi:
        return None
    for k in have:
        if lo <= k <= hi:
            return k
    mid = (lo + hi) // 2
    for k in sorted(range(lo, hi + 1), key=lambda k_: (k_ % 4 != 0, abs(k_ - mid))):
        return k
    return None


class Placed(NamedTuple):
    index: int          # row of the target table
    co: int
    tap: Tuple[int, int]
    a: float            # what the convolution itself must produce there: pre - bias
    s: float
    chunks: Tuple[float, float, float]
    channels: Tuple[int, int, int]
    pre: float          # the value in front of the activation / tail


class ConvCase(NamedTuple):
    dt: str
    flavour: str
    epilogue: str       # "none" | "relu" | "lrelu" | "res"
    slope: float
    x: torch.Tensor               # (n, cin, h, w) fp32, every value representable in the 16-bit type
    weight: torch.Tensor          # (cout, cin, k, k) fp32, every value representable in the 16-bit type
    bias: torch.Tensor            # (cout,) fp32, powers of two
    skip: Optional[torch.Tensor]  # (n, cout, h, w) fp32, representable in the 16-bit type ("res")
    scale: Optional[torch.Tensor]  # (n, cout) fp32, powers of two ("res")
    acc: torch.Tensor             # (n, cout, h, w) fp32: the convolution alone (exact)
    pre: torch.Tensor             # acc + bias (exact)
    want32: torch.Tensor          # the epilogue of pre in fp32 (exact); the 16-bit answer is want32.to(DT[dt])
    hit: torch.Tensor             # (n, cout, h, w) int64: the table row that lands there, -1 elsewhere
    placed: Tuple[Placed, ...]

    def nhwc16(self, t: torch.Tensor) -> torch.Tensor:
        return t.permute(0, 2, 3, 1).contiguous().to(DT[self.dt])

    def want16(self) -> torch.Tensor:
        """(n, h, w, cout) in the 16-bit type: the one right answer"""
        return self.nhwc16(self.want32)


def _final_of(v: float, epilogue: str) -> float:
    return max(v, 0.0) if epilogue == "relu" else v


def _pre_of(v: float, epilogue: str, slope: float, dt: str, scale: float) -> Optional[Tuple[float, float]]:
    """(value in front of the epilogue, skip value) so that the epilogue gives v (for ReLU: max(v, 0)); None if impossible in fp32"""
    if epilogue in ("none", "relu"):
        return v, 0.0
    if epilogue == "lrelu":
        pre = v if v >= 0 else v / slope
        return (pre, 0.0) if _exact32(pre) else None
    sk = math.copysign(_pow2_in(dt, _exp_of(v) - 2), v) if v != 0.0 else 0.25
    d = v - sk
    pre = d / scale
    if not (_exact32(d) and _exact32(pre)) or float(Fraction(sk) + Fraction(scale) * Fraction(pre)) != v:
        return None
    return pre, sk


def _scale_of(n: int, co: int) -> float:
    return 2.0 ** ((n + co) % 4 - 2)


def conv_cases(dt: str, shape: Tuple[int, int, int], sources: Sequence[Tuple[int, int, int]], flavour: str = "single",
               epilogue: str = "none", slope: float = 0.25, cout: int = 64, cin: int = 64, ksize: int = 3,
               table: Optional[Tuple[torch.Tensor, List[str]]] = None) -> List[ConvCase]:
    """Convolutions (stride 1, zero padding ksize // 2) whose exact results put the rows of the target table at pixels around
    `sources` = [(sample, y, x), ..].  One case per page of the table (an output channel has one bias, so it can only hold
    targets that are exact beside that bias).

    "single": a source pixel holds `s` of every scale group in that group's three input channels, and the weights of (co, tap)
    hold one target's three chunks in those channels: the target appears at the output pixel that reads the source through
    that tap, i.e. a source stamps up to ksize^2 x cout targets around itself.  Sources of one sample must lie at least
    ksize pixels apart (their stamps must not overlap).
    "three": chunk j sits at tap (centre row, centre - 1 + j) of the group's input channel j, and `sources` are the TARGET
    pixels: the pixels left of, at and right of one hold `s` in channel 0, 1, 2 of every group (a target in the first or
    last column is left out); one target per output channel and page.
    "res": out = skip + scale[n, co] * (conv + bias); the scale depends on the sample, so all sources share one sample."""
    assert flavour in ("single", "three") and epilogue in ("none", "relu", "lrelu", "res")
    assert cin % 16 == 0 or cin >= 3
    n, h, w = shape
    V, labels = table if table is not None else targets(dt)
    vals = V.double().tolist()
    kc = ksize // 2
    for (a_, ya, xa) in sources:
        assert 0 <= a_ < n and 0 <= ya < h and 0 <= xa < w, "source outside the tensor"
    if flavour == "single":
        for i, (a_, ya, xa) in enumerate(sources):
            for (b_, yb, xb) in sources[i + 1:]:
                assert a_ != b_ or max(abs(ya - yb), abs(xa - xb)) >= ksize, "stamps of two sources overlap"
    if epilogue == "res":
        assert len({s_[0] for s_ in sources}) == 1, "the tail's scale depends on the sample: one sample per case"
    sn = sources[0][0]
    taps = [(kc, kc)] + [(ky, kx) for ky in range(ksize) for kx in range(ksize) if (ky, kx) != (kc, kc)]
    if flavour == "three":
        taps = [(kc, kc)]           # (the slot; the chunks sit at (kc, kc - 1 + j))
    # triplets of input channels inside one 16-channel block (one k-step of the 16-bit MFMA)
    trip = [(16 * b + 3 * t, 16 * b + 3 * t + 1, 16 * b + 3 * t + 2) for b in range(max(cin // 16, 1)) for t in range(5)
            if 16 * b + 3 * t + 2 < cin]
    todo = list(range(len(vals)))
    cases: List[ConvCase] = []
    while todo:
        chan_bias: List[float] = []
        chan_used: List[int] = []
        ks: List[int] = []
        placed: List[Placed] = []
        skips = {}
        left = []
        for i in todo:
            v = vals[i]
            got = None
            # the scale of the tail is a property of (sample, channel): try the channels in turn
            # (existing ones first, then one of the next four unopened ones: their scales are 1/4, 1/2, 1, 2)
            cands = list(range(len(chan_bias))) + list(range(len(chan_bias), min(len(chan_bias) + 4, cout)))
            for co in cands:
                pr = _pre_of(v, epilogue, slope, dt, _scale_of(sn, co))
                if pr is None:
                    continue
                pre, sk = pr
                if co < len(chan_bias):
                    if chan_used[co] >= len(taps):
                        continue
                    b = chan_bias[co]
                else:
                    b = math.copysign(2.0 ** (_exp_of(pre) - 3), pre) if pre != 0.0 else 0.5
                a = pre - b
                if not _exact32(a) or float(Fraction(a) + Fraction(b)) != pre:
                    continue
                if a != 0.0 and not (0 < ((struct.unpack("<I", struct.pack("<f", a))[0] >> 23) & 0xFF) < 255):
                    continue
                ch = split3(a)
                k = _scale_for(dt, ch, ks)
                if k is None or (k not in ks and len(ks) >= len(trip)):
                    continue
                if k not in ks:
                    ks.append(k)
                while co > len(chan_bias):      # channels skipped on the way stay open for later targets
                    chan_bias.append(0.5)
                    chan_used.append(0)
                if co == len(chan_bias):
                    chan_bias.append(b)
                    chan_used.append(0)
                tap = taps[chan_used[co]]
                chan_used[co] += 1
                s = 2.0 ** k
                got = Placed(i, co, tap, a, s, tuple(c / s for c in ch), trip[ks.index(k)], pre)
                skips[(co, tap)] = sk
                break
            if got is None:
                left.append(i)
            else:
                placed.append(got)
        if not placed:
            break                       # (targets no page can hold under this epilogue, e.g. -fp32 max / slope)
        todo = left
        weight = torch.zeros(cout, cin, ksize, ksize, dtype=torch.float64)
        bias = torch.tensor(chan_bias + [0.5] * (cout - len(chan_bias)), dtype=torch.float64)
        for pl in placed:
            for j in range(3):
                ky, kx = pl.tap if flavour == "single" else (kc, kc - 1 + j)
                weight[pl.co, pl.channels[j], ky, kx] = pl.chunks[j]
        x = torch.zeros(n, cin, h, w, dtype=torch.float64)
        hit = torch.full((n, cout, h, w), -1, dtype=torch.int64)
        skip = None
        scale = None
        if epilogue == "res":
            scale = torch.tensor([[_scale_of(a_, co) for co in range(cout)] for a_ in range(n)], dtype=torch.float64)
            # away from the targets: a power of two near the channel's bias, so that skip + scale * bias is exact as well
            near = torch.tensor([_pow2_in(dt, _exp_of(b_) + 2) for b_ in bias.tolist()], dtype=torch.float64)
            near[1::2] *= -1.0
            skip = near.view(1, cout, 1, 1).expand(n, cout, h, w).clone()
        for (a_, ys, xs) in sources:
            if flavour == "three" and not (0 <= xs - 1 and xs + 1 < w):
                continue                  # a stamp the image edge would cut is left out: no partial sums anywhere
            for gi, k in enumerate(ks):
                for j in range(3):
                    if flavour == "single":
                        x[a_, trip[gi][j], ys, xs] = 2.0 ** k
                    elif 0 <= xs - 1 + j < w:
                        x[a_, trip[gi][j], ys, xs - 1 + j] = 2.0 ** k
            for pl in placed:
                if flavour == "single":
                    yo, xo = ys - (pl.tap[0] - kc), xs - (pl.tap[1] - kc)
                    if not (0 <= yo < h and 0 <= xo < w):
                        continue
                else:
                    yo, xo = ys, xs
                hit[a_, pl.co, yo, xo] = pl.index
                if skip is not None:
                    skip[a_, pl.co, yo, xo] = skips[(pl.co, pl.tap)]
        acc64 = F.conv2d(x, weight, None, 1, kc)
        pre64 = acc64 + bias.view(1, -1, 1, 1)
        if epilogue == "relu":
            want64 = torch.relu(pre64)
        elif epilogue == "lrelu":
            want64 = torch.where(pre64 >= 0, pre64, pre64 * slope)
        elif epilogue == "res":
            want64 = skip + scale.view(n, cout, 1, 1) * pre64
        else:
            want64 = pre64
        cases.append(ConvCase(dt, flavour, epilogue, slope, x.float(), weight.float(), bias.float(),
                              None if skip is None else skip.float(), None if scale is None else scale.float(),
                              acc64.float(), pre64.float(), want64.float(), hit, tuple(placed)))
    return cases


def final_values(case: ConvCase, table: torch.Tensor) -> torch.Tensor:
    """what the table rows that land in a case become: the row itself (-0 as +0), or max(row, 0) behind a ReLU; as (n, cout, h, w) fp32 with
    the case's own values where nothing lands (so that it compares equal to want32 everywhere)"""
    out = case.want32.clone()
    m = case.hit >= 0
    v = table[case.hit[m]] + 0.0      # (a -0 target arrives as +0: the accumulator starts at +0, and x + (-x) = +0)
    out[m] = torch.relu(v) if case.epilogue == "relu" else v
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# elementwise operands: r * scale[n, c] + x == V exactly
# ---------------------------------------------------------------------------------------------------------------------------
def trunc16(v: torch.Tensor, dt: str) -> torch.Tensor:
    """the neighbour of v in the 16-bit type towards zero (largest finite value beyond the range), as fp32"""
    return round_to(v, dt, "truncate").float()


def scale_residual_case(dt: str, n: int, h: int, w: int, table: Optional[torch.Tensor] = None, page: int = 0):
    """(r, scale, x, want32): r, x (n, 64, h, w) fp32 representable in the 16-bit type, scale (n, 64) fp32 dyadic, with
    r * scale + x exact in fp32 and equal to a table value (times r) wherever r != 0.  Channel c of sample a carries row
    (page * n * 64 + a * 64 + c) of the table (wrapped around): x = r * trunc16(V), scale = V - trunc16(V); r cycles through
    0, 1, 2, 1/2 along the pixels where V's neighbours allow it (range top and subnormals: 0 and 1 only)."""
    V = targets(dt)[0] if table is None else table
    idx = (page * n * 64 + torch.arange(n * 64)) % V.numel()
    v = V[idx].double().view(n, 64, 1, 1)
    tr = trunc16(V, dt).double()[idx].view(n, 64, 1, 1)
    scale = (v - tr).view(n, 64)
    wide = (v.abs() < 2.0 ** (EMAX[dt] - 1)) & (v.abs() >= 2.0 ** (EMIN[dt] + 2))
    cyc = torch.tensor([0.0, 1.0, 2.0, 0.5], dtype=torch.float64)
    pix = torch.arange(h * w).view(1, 1, h, w)
    r = torch.where(wide, cyc[pix % 4].expand(n, 64, h, w), cyc[pix % 2].expand(n, 64, h, w))
    x = r * tr
    want = r * scale.view(n, 64, 1, 1) + x
    return r.float(), scale.float(), x.float(), want.float(), idx
