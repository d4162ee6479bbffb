"""Helper of tests/test_hip_product_probe.py (checked on the CPU by tests/test_product_probe_host.py): probes in which every output
element of a bf16-split kernel is ONE product x * w plus exact zeros, so that a lost plane product cannot average away.

The kernels (csrc/conv_x6.hip, conv3_x6s.hip, conv_x9.hip, dcnv2_il.hip, dcnv2_il2.hip, dcnv2_x9.hip, dcnv2_ws.hip, the split path
of conv_wgrad.hip) split each fp32 operand by TRUNCATION into hi + mid + lo (three bf16 numbers, bit-exact) and accumulate six of the
nine plane products in fp32 (nine: nprod = 9 / bf16x9).  `split3` restates the split on uint32 bit patterns, `emulate` sums a chosen
set of plane products in float64.

Sizes under truncation: |mid| < 2^-7 |x|, |lo| < 2^-15 |x|, so the dropped products mid*lo + lo*mid + lo*lo are below
2 * 2^-22 (1 - 2^-8) + 2^-30 < 2^-21 of |x * w| together, EACH of the first two below 2^-22 (not 2^-23: tests/test_product_probe_host.py
shows an operand pair at 2^-21.02).

Probe classes (significant bits of x / of w): A 8 / 24 (live: hh hm hl), B 24 / 8 (hh mh lh), C 16 / 16 (hh hm mh mm), D 24 / 24
(all nine).  In A, B, C no dropped product is non-zero: a correct kernel is off by its accumulation's rounding only.

Bounds, u = 2^-24, 2 u allowed per addition (the rounding inside the matrix instruction is not documented as to-nearest):
  * one product, A / B / C, and D with nine products:  |out - x w| <= 16 u |x w|   (eight additions of nine terms)
  * D with six products:                               (2^-21 + 16 u) |x w|
  * the fp32-MFMA routes ("direct", DCN mode "native"): 2 u |x w|
  * a probe-valued DCNv2 mask adds the rounding of mask * sample: + 2 u
  * dense: |out - ref64| <= 2 (K + 8) u sum |x||w|  (+ 2^-21 sum |x||w| with six products), K the length of the reduction.
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Sequence, Tuple

import numpy as np

U = 2.0 ** -24
NAMES = ("h", "m", "l")
ALL9 = tuple(itertools.product(range(3), range(3)))                 # (plane of x, plane of w)
SIX = tuple(p for p in ALL9 if p[0] + p[1] <= 2)                    # hh hm hl mh mm lh
DROPPED = tuple(p for p in ALL9 if p[0] + p[1] > 2)                 # ml lm ll
DROP_REL = 2.0 ** -21                                               # the three dropped products together, relative to |x w|
CLASSES = {"A": (8, 24), "B": (24, 8), "C": (16, 16), "D": (24, 24)}
LIVE = {"A": ((0, 0), (0, 1), (0, 2)), "B": ((0, 0), (1, 0), (2, 0)), "C": ((0, 0), (0, 1), (1, 0), (1, 1)), "D": ALL9}


def pname(p) -> str:
    return NAMES[p[0]] + NAMES[p[1]]


# ------------------------------------------------------------------------------------------ the split
def bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def floats(u: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


_TOP = np.uint32(0xFFFF0000)


def split3(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """eavsr_split2 (csrc/mfma.h): hi = the top 16 bits of x, mid = the top 16 bits of x - hi, lo = x - hi - mid (fp32
    subtractions, both exact)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = floats(bits(x) & _TOP)
    r = x - hi
    mid = floats(bits(r) & _TOP)
    return hi, mid, r - mid


def split3_rne_hi(x: np.ndarray):
    """MUTANT: hi rounded to nearest even, mid and lo still those of the truncated hi"""
    u = bits(x).astype(np.uint64)
    hi = floats(((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32))
    return (hi,) + split3(x)[1:]


def round_bf16(x: np.ndarray) -> np.ndarray:
    return split3_rne_hi(x)[0]


def emulate(x, w, planes: Sequence[Tuple[int, int]] = SIX, split_x=split3, split_w=split3) -> np.ndarray:
    """float64 sum of the chosen plane products of x * w (elementwise)"""
    px, pw = split_x(np.asarray(x, np.float32)), split_w(np.asarray(w, np.float32))
    out = np.zeros(np.broadcast(px[0], pw[0]).shape, np.float64)
    for i, j in planes:
        out += px[i].astype(np.float64) * pw[j].astype(np.float64)
    return out


# ------------------------------------------------------------------------------------------ probe values
def probe(nbits: int, shape, rng: np.random.Generator, random_mantissa: bool = False) -> np.ndarray:
    """normal fp32 numbers, random sign, exponent in [-12, 12], `nbits` significant bits in 8-bit fields; every field has its top
    and its bottom bit set (the first field's top bit is the implicit one) and the fields below the first are near their maximum
    (half of them 0xFF).  A quarter of the first fields are the smallest (0x81): the low planes are then largest against x."""
    shape = tuple(np.atleast_1d(shape))
    sign = rng.integers(0, 2, shape, dtype=np.uint32) << 31
    expo = (rng.integers(-12, 13, shape) + 127).astype(np.uint32) << 23

    def low_field():
        f = np.where(rng.random(shape) < 0.5, 0x3F, rng.integers(0x30, 0x40, shape))
        return (0x81 | (f << 1)).astype(np.uint32)
    f1 = np.where(rng.random(shape) < 0.25, 0, rng.integers(0, 64, shape)).astype(np.uint32) << 1 | 1       # 7 stored bits
    mant = f1 << 16
    if nbits >= 16:
        mant = mant | (low_field() << 8)
    if nbits >= 24:
        mant = mant | low_field()
    if random_mantissa:
        mant = rng.integers(0, 1 << 23, shape).astype(np.uint32)
    return floats(sign | expo | mant.astype(np.uint32))


def probe_pair(cls: str, xshape, wshape, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """(x values, w values) of a class; class D: the structured fields for the even flat indices, random mantissas for the odd"""
    rng = np.random.default_rng([seed, ord(cls)])
    bx, bw = CLASSES[cls]
    x, w = probe(bx, xshape, rng), probe(bw, wshape, rng)
    if cls == "D":
        for v in (x, w):
            flat = v.reshape(-1)
            flat[1::2] = probe(24, flat[1::2].shape, rng, random_mantissa=True)
    return x, w


def one_product_bound(cls: str, nprod: int = 6, native: bool = False, mask: bool = False) -> float:
    """relative to |x w| (|mask x w|)"""
    b = 2 * U if native else 16 * U + (DROP_REL if (cls == "D" and nprod == 6) else 0.0)
    return b + (2 * U if mask else 0.0)


def dense_bound(K: int, nprod: int = 6, native: bool = False) -> float:
    """relative to sum |x||w| of the output element"""
    return 2 * (K + 8) * U + (DROP_REL if (nprod == 6 and not native) else 0.0)


# ------------------------------------------------------------------------------------------ mutants
def last_pair_taps(k: int) -> Tuple[int, ...]:
    """the taps of a layer's last tap pair (k-step): the last tap and the zero tap that pads k * k to an even count"""
    kk = k * k
    return tuple(t for t in (2 * ((kk + 1) // 2 - 1), 2 * ((kk + 1) // 2 - 1) + 1) if t < kk)


def mutants() -> Dict[str, callable]:
    """name -> f(x, w, tap, k, nprod) -> float64 emulation of a WRONG kernel (tap: the tap index of each element)"""
    def planes_of(nprod):
        return ALL9 if nprod == 9 else SIX
    m = {}
    for p in ALL9:
        m["no_" + pname(p)] = lambda x, w, tap, k, nprod, p=p: emulate(x, w, [q for q in planes_of(nprod) if q != p])
    m["rne_hi"] = lambda x, w, tap, k, nprod: emulate(x, w, planes_of(nprod), split3_rne_hi, split3_rne_hi)
    m["bf16_once"] = lambda x, w, tap, k, nprod: round_bf16(x).astype(np.float64) * round_bf16(w).astype(np.float64)
    m["nine_as_six"] = lambda x, w, tap, k, nprod: emulate(x, w, SIX)

    def last_lo(x, w, tap, k, nprod):
        full = emulate(x, w, planes_of(nprod))
        cut = emulate(x, w, [q for q in planes_of(nprod) if q[1] != 2])      # the weight pack's lo plane zeroed
        return np.where(np.isin(tap, last_pair_taps(k)), cut, full)
    m["last_pair_lo"] = last_lo
    return m


# what the suite's metric before this file (2e-5 max|ref| on randn data) can and cannot see
GROSS = ("no_hh", "no_hm", "no_mh", "rne_hi", "bf16_once")
SUBTLE = ("no_hl", "no_lh", "no_mm", "no_ml", "no_lm", "no_ll", "nine_as_six", "last_pair_lo")
# no fp32 output can show these against a bound: ml + lm + ll < 8 u, below the 16 u an honest nine-product sum is allowed.  The
# nine-product runs are held to `nine_minus_six` instead; ll (< 2^-30, a 64th of an output ulp) is beyond any test of the output.
BELOW_BOUND = ("no_ml", "no_lm", "no_ll", "nine_as_six")


def nine_minus_six(out9, out6, x, w) -> Tuple[float, float]:
    """(mean of (out9 - out6) / (x w), mean of the dropped products / (x w)) over class-D elements: a nine-product run that
    accumulates mid*lo and lo*mid differs from the six-product run of the same kernel by them on average (the roundings of the two
    runs are those of the same additions and do not correlate with the products' size); without both the first figure is at most
    half the second.  The test asks for 3/4."""
    xw = np.asarray(x, np.float64) * np.asarray(w, np.float64)
    got = (np.asarray(out9, np.float64) - np.asarray(out6, np.float64)) / xw
    want = emulate(x, w, DROPPED) / xw
    return float(got.mean()), float(want.mean())


# ------------------------------------------------------------------------------------------ one-hot schedules
def conv_schedule(k: int, cin: int, cout: int) -> List[Tuple[np.ndarray, np.ndarray]]:
    """[(ci[co], tap[co])] per weight tensor: output channel co of tensor j holds pair j * cout + co of the layer's cin * k * k
    (channel, tap) pairs, pair p = (channel p // k^2, tap p % k^2); -1: the channel's weights are all zero (past the last pair)"""
    kk = k * k
    total = cin * kk
    out = []
    for j in range(-(-total // cout)):
        p = j * cout + np.arange(cout)
        live = p < total
        out.append((np.where(live, p // kk, -1), np.where(live, p % kk, -1)))
    return out


def onehot_weight(k: int, cin: int, ci: np.ndarray, tap: np.ndarray, values: np.ndarray) -> np.ndarray:
    """(cout, cin, k, k) fp32, w[co, ci[co], tap[co]] = values[co], +0 elsewhere"""
    cout = len(ci)
    w = np.zeros((cout, cin, k * k), np.float32)
    live = ci >= 0
    w[np.arange(cout)[live], ci[live], tap[live]] = values[live]
    return w.reshape(cout, cin, k, k)


def onehot_expected(x: np.ndarray, k: int, ci: np.ndarray, tap: np.ndarray, values: np.ndarray, dy=None, dx=None, mask=None):
    """the operands of the one product behind every output element of the "same" cross-correlation of x (n, cin, h, w) with
    onehot_weight: (xs, ws, inside), each (n, cout, h, w); out = ws * xs (float64) where inside, exactly zero elsewhere.
    dy, dx: integer DCNv2 offsets (n, cout, h, w) of each channel's tap; mask: its modulation, already gathered per cout."""
    n, cin, h, w = x.shape
    cout = len(ci)
    r = k // 2
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    xs = np.zeros((n, cout, h, w), np.float32)
    inside = np.zeros((n, cout, h, w), bool)
    for co in range(cout):
        if ci[co] < 0:
            continue
        sy = yy[None] + (tap[co] // k - r) + (0 if dy is None else dy[:, co])
        sx = xx[None] + (tap[co] % k - r) + (0 if dx is None else dx[:, co])
        ok = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
        g = x[np.arange(n)[:, None, None], ci[co], np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
        xs[:, co] = np.where(ok, g, 0)
        inside[:, co] = ok
    ws = np.broadcast_to(np.where(ci >= 0, values, 0).astype(np.float32)[None, :, None, None], xs.shape)
    return xs, ws, inside


def wgrad_positions(h: int, w: int, th: int = 8, tw: int = 32) -> List[Tuple[int, int]]:
    """every position of the first th x tw tile, then the first row and the first column of the ragged tiles behind it"""
    pos = [(y, x) for y in range(min(th, h)) for x in range(min(tw, w))]
    if h > th:
        pos += [(th, x) for x in range(min(tw + 1, w))]
    if w > tw:
        pos += [(y, tw) for y in range(min(th, h))]
    return pos


def wgrad_schedule(h: int, w: int, cout: int) -> List[np.ndarray]:
    """[(cout, 3) int array of (image, y, x)] per dY tensor: channel co of tensor j is non-zero at position j * cout + co of
    wgrad_positions (image = that index % 2), -1 past the last position"""
    pos = wgrad_positions(h, w)
    out = []
    for j in range(-(-len(pos) // cout)):
        a = np.full((cout, 3), -1, np.int64)
        for co in range(cout):
            p = j * cout + co
            if p < len(pos):
                a[co] = (p % 2, *pos[p])
        out.append(a)
    return out


def wgrad_onehot(n: int, h: int, w: int, where: np.ndarray, values: np.ndarray) -> np.ndarray:
    cout = len(where)
    dy = np.zeros((n, cout, h, w), np.float32)
    for co, (i, y, x) in enumerate(where):
        if i >= 0:
            dy[i % n, co, y, x] = values[co]
    return dy


def wgrad_expected(x: np.ndarray, where: np.ndarray, values: np.ndarray, k: int = 3):
    """dW[co, ci, t] = dY[co, p] * x[ci, p + t]: (xs, ws, inside), each (cout, cin, k, k)"""
    n, cin, h, w = x.shape
    cout, r = len(where), k // 2
    xs = np.zeros((cout, cin, k, k), np.float32)
    inside = np.zeros((cout, cin, k, k), bool)
    for co, (i, y, xx) in enumerate(where):
        if i < 0:
            continue
        for ky in range(k):
            for kx in range(k):
                sy, sx = y + ky - r, xx + kx - r
                if 0 <= sy < h and 0 <= sx < w:
                    xs[co, :, ky, kx] = x[i % n, :, sy, sx]
                    inside[co, :, ky, kx] = True
    ws = np.broadcast_to(np.where(where[:, 0] >= 0, values, 0).astype(np.float32)[:, None, None, None], xs.shape)
    return xs, ws, inside


# ------------------------------------------------------------------------------------------ checks shared by host and GPU tests
def rel_error(out, xs, ws, inside) -> float:
    """max |out - x w| / |x w| over the elements that hold a product"""
    ref = xs.astype(np.float64) * ws.astype(np.float64)
    live = inside & (ref != 0)
    if not live.any():
        return 0.0
    return float((np.abs(np.asarray(out, np.float64) - ref)[live] / np.abs(ref[live])).max())


def zeros_ok(out, xs, ws, inside) -> bool:
    """every element without a product is +0.0 or -0.0 (never NaN, never a leaked value)"""
    dead = ~(inside & (ws != 0))
    return bool((np.asarray(out)[dead] == 0).all())


def dense_inputs(n: int, cin: int, cout: int, h: int, w: int, k: int, seed: int = 0):
    """full-mantissa operands whose per-input-channel scales spread over 2^-20 .. 2^20 (the weights' the inverse): fp32 x, w"""
    rng = np.random.default_rng([seed, cin, cout, k])
    s = np.linspace(-20, 20, cin).round()
    rng.shuffle(s)
    x = (rng.standard_normal((n, cin, h, w)) * 2.0 ** s[None, :, None, None]).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, k, k)) * 2.0 ** -s[None, :, None, None]).astype(np.float32)
    return x, wt


def is_normal(v: np.ndarray) -> bool:
    """finite, and no non-zero value below the smallest normal fp32"""
    a = np.abs(np.asarray(v, np.float64))
    return bool(np.isfinite(a).all() and ((a == 0) | ((a >= 2.0 ** -126) & (a < 2.0 ** 128))).all())
