"""The contract of the Winograd convolution kernel (csrc/conv_wino6.hip: F(4x4,3x3), routes wino4, and F(2x2,5x5), route wino5),
restated in numpy from the comments at the head of that file and from pack_wino6_kernel -- nothing here imports the library.
Helper of tests/test_wino4_contract_host.py (CPU) and tests/test_hip_wino4_contract.py (GPU); DESIGN.md 4b is the prose.

  matrices   BT, g_matrix(R), at_matrix(M): the points 0, +-1, +-2, inf
  geometry   Geo(k): the 8 x 64 (4 x 32) workgroup tile, the 4 x 4 (2 x 2) Winograd tile, tiles_containing()
  reference  ref64 / bound / Conv: the direct fp64 convolution with conv2d's epilogue, and the per-pixel allowance K u E + epilogue
  emulation  emulate32: the algorithm in fp32, elementwise numpy only (bit-reproducible); MUTANTS: emulations wrong in one way each
  checkers   check_local / check_impulse / check_nonfinite / check_part / check_pieces (new) and old_global / old_part (what
             tests/test_hip_ops.py asserts), applied alike to the emulation, its mutants and the kernel
  cases      CASES: the shapes and inputs both test files walk
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

U = 2.0 ** -24                     # unit roundoff of fp32
C0 = 14                            # rounding depth of the three transforms: 2 x 3 (input) + 1 (U) + 1 (product) + 2 x 3 (output)
K_FACTOR = 4.0                     # the kernel's legitimate other association order (MFMA k-steps, packed pairs, slot pairing)
# K = K_FACTOR x the largest err / (u E) emulate32 reaches over CASES x INPUT_KINDS; pinned by test_K_is_four_times_the_emulation
K_EMULATION_RATIO = 3.3428647
K = K_FACTOR * K_EMULATION_RATIO
EPI = 2.0                          # u-multiples allowed per epilogue term (one rounding each, doubled for second order)
SUM_DEPTH = 12                     # depth of the channel-sum reduction (2 in the lane, 4 rows, 1, 4 shuffles, 1 across waves)
LINE_DEPTH = 6                     # depth of a border piece's reduction (2 in the lane + 4 shuffles; 4 for a column piece)
SLOPE = np.float32(0.1)

POINTS = (0.0, 1.0, -1.0, 2.0, -2.0)
SCALES = (1 / 4, -1 / 6, -1 / 6, 1 / 24, 1 / 24)
BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
               [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64)


def g_matrix(r: int) -> np.ndarray:
    """6 x r: row p = scale_p (1, p, p^2, ..) for the finite points, the unit vector of the highest power for infinity"""
    g = np.zeros((6, r))
    for i, (p, s) in enumerate(zip(POINTS, SCALES)):
        g[i] = [s * p ** e for e in range(r)]
    g[5, r - 1] = 1.0
    return g


def at_matrix(m: int) -> np.ndarray:
    """m x 6: row e = (p^e for the finite points, 1 in the last row for infinity)"""
    a = np.zeros((m, 6))
    for e in range(m):
        a[e, :5] = [p ** e for p in POINTS]
    a[m - 1, 5] = 1.0
    return a


G3, G5, AT4, AT2 = g_matrix(3), g_matrix(5), at_matrix(4), at_matrix(2)


@dataclass(frozen=True)
class Geo:
    k: int

    @property
    def m(self):            # outputs per Winograd tile side
        return 7 - self.k

    @property
    def pad(self):
        return self.k // 2

    @property
    def toh(self):          # workgroup tile: 2 x 16 Winograd tiles
        return 2 * self.m

    @property
    def tow(self):
        return 16 * self.m

    def wtiles(self, h, w):
        return -(-h // self.toh), -(-w // self.tow)

    def tiles(self, h, w):
        return -(-h // self.m), -(-w // self.m)

    def tiles_containing(self, y: int, x: int, h: int, w: int) -> List[Tuple[int, int, int, int]]:
        """(ty, tx, i, j): the Winograd tiles whose 6 x 6 patch holds input pixel (y, x), and its position in that patch.  Tile
        (ty, tx) writes output rows m ty .. m ty + m - 1 and reads input rows m ty - pad .. m ty - pad + 5."""
        ty_n, tx_n = self.tiles(h, w)
        out = []
        for ty in range(ty_n):
            i = y - (self.m * ty - self.pad)
            if not 0 <= i < 6:
                continue
            for tx in range(tx_n):
                j = x - (self.m * tx - self.pad)
                if 0 <= j < 6:
                    out.append((ty, tx, i, j))
        return out

    def tile_mask(self, pixels: Sequence[Tuple[int, int]], h: int, w: int) -> np.ndarray:
        """(h, w) bool: the output pixels of every Winograd tile whose patch holds one of `pixels`"""
        mask = np.zeros((h, w), bool)
        for y, x in pixels:
            for ty, tx, _, _ in self.tiles_containing(y, x, h, w):
                mask[self.m * ty:self.m * ty + self.m, self.m * tx:self.m * tx + self.m] = True
        return mask


# ------------------------------------------------------------------------------------------ epilogue pieces
def act_of(v: np.ndarray, act: Optional[str], slope=SLOPE) -> np.ndarray:
    """eavsr_act's rule: v where v > 0 or v is a NaN, else v (*) s with s = 1 / 0 / slope and 0 (*) anything = +0"""
    s = {None: 1.0, "relu": 0.0, "lrelu": float(slope)}[act]
    if s == 1.0:
        return v
    with np.errstate(invalid="ignore"):
        z = np.zeros_like(v) if s == 0.0 else v * v.dtype.type(s)
        return np.where(~(v <= 0), v, z)


def pixel_shuffle2(a: np.ndarray) -> np.ndarray:
    n, c, h, w = a.shape
    return a.reshape(n, c // 4, 2, 2, h, w).transpose(0, 1, 4, 2, 5, 3).reshape(n, c // 4, 2 * h, 2 * w)


def pixel_unshuffle2(a: np.ndarray) -> np.ndarray:
    n, c, h2, w2 = a.shape
    return a.reshape(n, c, h2 // 2, 2, w2 // 2, 2).transpose(0, 1, 3, 5, 2, 4).reshape(n, 4 * c, h2 // 2, w2 // 2)


def _direct(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    k, p = w.shape[-1], w.shape[-1] // 2
    n, _, h, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
    out = np.zeros((n, w.shape[0], h, wd), x.dtype)
    for i in range(k):
        for j in range(k):
            out += np.einsum("oc,nchw->nohw", w[:, :, i, j], xp[:, :, i:i + h, j:j + wd])
    return out


def _patches(x: np.ndarray, k: int, mode: str = "constant") -> np.ndarray:
    """(n, c, TY, TX, 6, 6): every Winograd tile's input patch, zeros (mode "constant") outside the image"""
    g = Geo(k)
    n, c, h, w = x.shape
    ty, tx = g.tiles(h, w)
    xp = np.pad(x, ((0, 0), (0, 0), (g.pad, g.m * ty + k - 1 - g.pad - h), (g.pad, g.m * tx + k - 1 - g.pad - w)), mode=mode)
    win = np.lib.stride_tricks.sliding_window_view(xp, (6, 6), axis=(2, 3))
    return win[:, :, ::g.m, ::g.m]


def _untile(y: np.ndarray, h: int, w: int) -> np.ndarray:
    """(n, co, TY, TX, m, m) -> (n, co, h, w)"""
    n, co, ty, tx, m, _ = y.shape
    return y.transpose(0, 1, 2, 4, 3, 5).reshape(n, co, ty * m, tx * m)[:, :, :h, :w]


def winograd_abs(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """E: the Winograd expression on absolute values, |A^T| [ sum_ci (|G||g||G^T|) .* (|B^T||d||B|) ] |A|, per output pixel (fp64)"""
    k = w.shape[-1]
    gm, at = np.abs(g_matrix(k)), np.abs(at_matrix(7 - k))
    bt = np.abs(BT)
    d = np.abs(_patches(x.astype(np.float64), k))
    v = np.einsum("ai,nctsij,bj->nctsab", bt, d, bt, optimize=True)
    u = np.einsum("ai,ocij,bj->ocab", gm, np.abs(w.astype(np.float64)), gm, optimize=True)
    m = np.einsum("ocab,nctsab->notsab", u, v, optimize=True)
    y = np.einsum("ea,notsab,fb->notsef", at, m, at, optimize=True)
    return _untile(y, x.shape[2], x.shape[3])


def winograd64(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """the algorithm itself in fp64 (host check that the matrices and the geometry above ARE a convolution)"""
    k = w.shape[-1]
    gm, at = g_matrix(k), at_matrix(7 - k)
    d = _patches(x.astype(np.float64), k)
    v = np.einsum("ai,nctsij,bj->nctsab", BT, d, BT, optimize=True)
    u = np.einsum("ai,ocij,bj->ocab", gm, w.astype(np.float64), gm, optimize=True)
    m = np.einsum("ocab,nctsab->notsab", u, v, optimize=True)
    return _untile(np.einsum("ea,notsab,fb->notsef", at, m, at, optimize=True), x.shape[2], x.shape[3])


@dataclass
class Result:
    ref: np.ndarray          # what the launch returns, fp64 (shuffled layout with shuffle)
    bound: np.ndarray        # per-pixel allowance on |out - ref|
    pre: np.ndarray          # act(conv + bias): what the channel sums and border pieces add up (never shuffled)
    bound_pre: np.ndarray
    E: np.ndarray


class Conv:
    """conv64 and E of one (x, w), computed once; epilogue() derives reference and bound for any epilogue of conv2d"""

    def __init__(self, x: np.ndarray, w: np.ndarray, x_err: Optional[np.ndarray] = None):
        """x_err: per-pixel bound on what the kernel's own input differs from x by (the fused prologue forms its input in fp32;
        fused_input).  It goes through the convolution like any input perturbation: |A^T| [sum |U| .* (|B^T| x_err |B|)] |A|."""
        self.x, self.w = x, w
        self.conv = _direct(x.astype(np.float64), w.astype(np.float64))
        self.E = winograd_abs(x, w)
        self.E_in = None if x_err is None else winograd_abs(x_err, w)

    def epilogue(self, bias=None, act=None, slope=SLOPE, residual=None, res_scale=None, shuffle=False, k_factor: float = K) -> Result:
        """out = residual + res_scale[n, co] * act(conv + bias) (ops.conv2d's docstring; res_scale = 1, residual = 0 when absent).
        Allowance: K u E for the convolution; then ONE rounding per epilogue operation, each at most u times the magnitude it
        produces -- the bias add (<= |conv| + |bias|; |conv| <= E), the slope product (|pre|), the scale product (|scale pre|), the
        residual add (|result| <= |scale pre| + |residual|) -- allowed EPI = 2 u each.  act is 1-Lipschitz (0 <= slope <= 1), the
        scale multiplies what came before it."""
        y = self.conv + (0.0 if bias is None else bias.astype(np.float64)[None, :, None, None])
        pre = act_of(y, act, slope)
        b_pre = k_factor * U * self.E
        if self.E_in is not None:
            b_pre = b_pre + self.E_in
        if bias is not None:
            b_pre = b_pre + EPI * U * (np.abs(bias.astype(np.float64))[None, :, None, None] + np.abs(y))
        if act == "lrelu":
            b_pre = b_pre + EPI * U * np.abs(pre)
        ref, b = pre, b_pre
        if res_scale is not None:
            s = res_scale.astype(np.float64)[:, :, None, None]
            ref, b = s * ref, np.abs(s) * b + EPI * U * np.abs(s * pre)
        if residual is not None:
            ref = ref + residual.astype(np.float64)
            b = b + EPI * U * (np.abs(residual.astype(np.float64)) + np.abs(ref))
        if shuffle:
            ref, b = pixel_shuffle2(ref), pixel_shuffle2(b)
        return Result(ref, b, pre, b_pre, self.E)


def fused_input(r: np.ndarray, scale: np.ndarray, x: np.ndarray):
    """the fused channel-attention prologue (lab build): the kernel convolves d = r * scale[n, c] + x, formed in fp32 in its input
    transform.  Returns d in fp64 and the bound on the fp32 d's distance from it: a product and a sum, u |r s| + u (|r s| + |x|), or
    one fma, u |r s + x|: at most 2 u (|r s| + |x|) either way."""
    rs = r.astype(np.float64) * scale.astype(np.float64)[:, :, None, None]
    return rs + x.astype(np.float64), 2 * U * (np.abs(rs) + np.abs(x.astype(np.float64)))


def ref64(x, w, bias=None, act=None, slope=SLOPE, residual=None, res_scale=None, shuffle=False) -> np.ndarray:
    return Conv(x, w).epilogue(bias, act, slope, residual, res_scale, shuffle).ref


def bound(x, w, bias=None, act=None, slope=SLOPE, residual=None, res_scale=None, shuffle=False) -> np.ndarray:
    return Conv(x, w).epilogue(bias, act, slope, residual, res_scale, shuffle).bound


# ------------------------------------------------------------------------------------------ the fp32 emulation and its mutants
MUTANTS = ("bt_lowbit", "leak", "leak_rows", "bf16_patch", "nan_zero", "clamp_halo")
SUM_MUTANTS = ("swap_part", "swap_pieces")
F32 = np.float32


def round_bf16(a: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)


def _in1d(d: np.ndarray, axis: int, five: np.float32) -> np.ndarray:
    d0, d1, d2, d3, d4, d5 = (np.take(d, i, axis) for i in range(6))
    f4, f2 = F32(4), F32(2)
    a, b, c, e = d4 - f4 * d2, d3 - f4 * d1, d4 - d2, d3 - d1
    t = [f4 * d0 + (d4 - five * d2), a + b, a - b, c + f2 * e, c - f2 * e, f4 * d1 + (d5 - five * d3)]
    return np.stack(t, axis)


def _out1d(m: np.ndarray, axis: int, k: int) -> np.ndarray:
    m0, m1, m2, m3, m4, m5 = (np.take(m, i, axis) for i in range(6))
    if k == 3:
        p1, p2, p3, p4 = m1 + m2, m1 - m2, m3 + m4, m3 - m4
        s = [m0 + p1 + p3, p2 + F32(2) * p4, p1 + F32(4) * p3, (p2 + F32(8) * p4) + m5]
    else:
        s = [m0 + (m1 + m2) + (m3 + m4), ((m1 - m2) + F32(2) * (m3 - m4)) + m5]
    return np.stack(s, axis)


def pack_u64(w: np.ndarray) -> np.ndarray:
    """U = G g G^T, (cout, cin, 6, 6), fp64"""
    gm = g_matrix(w.shape[-1])
    return np.einsum("ai,ocij,bj->ocab", gm, w.astype(np.float64), gm, optimize=True)


def pack_exact(m: np.ndarray) -> np.ndarray:
    """U of the weight 576 m for an INTEGER m, exactly: 24 G is an integer matrix, so G (576 m) G^T = (24 G) m (24 G)^T in integers
    (every factor 1/4, 1/6, 1/24 and their products divide out)"""
    g24 = np.rint(24 * g_matrix(m.shape[-1])).astype(np.int64)
    assert np.abs(g24 - 24 * g_matrix(m.shape[-1])).max() < 1e-12
    return np.einsum("ai,ocij,bj->ocab", g24, m.astype(np.int64), g24)


def check_pack(u32: np.ndarray, m: np.ndarray, what: str = "") -> None:
    """u32 (cout, cin, 6, 6) fp32, what a pack of the weight 576 m returned, against the exact integers: bit for bit wherever the
    exact value is not zero (an evaluation in double errs by < 2^-45 of the sum of its terms' magnitudes, far inside the fp32
    spacing of an integer below 2^24, so ONE rounding lands on it); where the terms cancel to zero, what is left is that
    evaluation's own residue (1/6 is no double), allowed 2^-45 of the terms' magnitudes.  A one-hot m has one term per position:
    nothing cancels, every position is bit for bit."""
    exact = pack_exact(m)
    g24 = np.abs(np.rint(24 * g_matrix(m.shape[-1]))).astype(np.int64)
    mag = np.einsum("ai,ocij,bj->ocab", g24, np.abs(m).astype(np.int64), g24)
    _fail(u32.dtype == np.float32 and u32.shape == exact.shape, f"{what}: {u32.dtype} {u32.shape}")
    nz = exact != 0
    bad = nz & (u32 != exact.astype(np.float32))
    _fail(not bad.any(), f"{what}: {int(bad.sum())} packed weights differ from G g G^T, first (co, ci, i, q) = "
                         f"{tuple(int(v) for v in np.argwhere(bad)[0]) if bad.any() else None}")
    res = ~nz & (np.abs(u32.astype(np.float64)) > 2.0 ** -45 * mag)
    _fail(not res.any(), f"{what}: {int(res.sum())} positions that cancel to zero hold more than a double evaluation's residue")


def emulate32(x, w, bias=None, act=None, slope=SLOPE, residual=None, res_scale=None, shuffle=False, mutant: Optional[str] = None,
              want_pre: bool = False):
    """The algorithm in fp32, every operation an elementwise numpy one: the input transform in two passes, U evaluated in fp64 and
    rounded once, fp32 products accumulated over cin in order, the output transform in two passes, conv2d's epilogue.  `mutant`
    makes it wrong in one way (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS, mutant
    k = w.shape[-1]
    g = Geo(k)
    n, cin, h, wd = x.shape
    x = np.ascontiguousarray(x, F32)
    if mutant == "bf16_patch":
        x = round_bf16(x)
    d = _patches(x, k, mode="edge" if mutant == "clamp_halo" else "constant")
    if mutant == "nan_zero":
        d = np.where(np.isnan(d), F32(0), d)
    five = F32(5 * (1 + 2.0 ** -16)) if mutant == "bt_lowbit" else F32(5)
    with np.errstate(invalid="ignore", over="ignore"):
        v = _in1d(_in1d(d, -2, five), -1, five)
        u = pack_u64(w).astype(F32)
        acc = np.zeros((n, w.shape[0]) + v.shape[2:], F32)
        for ci in range(cin):
            acc += u[None, :, ci, None, None] * v[:, None, ci]
        if mutant == "leak":
            acc = _leak(acc, g, h, wd)
        if mutant == "leak_rows":      # the lower tile row of a workgroup picks up 2^-20 of the upper one's accumulators
            acc = acc.copy()
            pairs = acc.shape[2] // 2
            acc[:, :, 1:2 * pairs:2] += F32(2.0 ** -20) * acc[:, :, 0:2 * pairs:2]
        y = _untile(_out1d(_out1d(acc, -2, k), -1, k), h, wd)
        if bias is not None:
            y = y + bias.astype(F32)[None, :, None, None]
        pre = act_of(y, act, slope)
        out = pre
        if res_scale is not None:
            out = out * res_scale.astype(F32)[:, :, None, None]
        if residual is not None:
            out = out + residual.astype(F32)
    if shuffle:
        out = pixel_shuffle2(out)
    return (out, pre) if want_pre else out


def _leak(acc: np.ndarray, g: Geo, h: int, w: int, grid: int = 256) -> np.ndarray:
    """a workgroup's second (third, ..) tile starts from 2^-20 x the accumulators its previous tile ended with: workgroup b of
    min(tiles, 256) walks the workgroup tiles b, b + grid, .. of the (image, row, column) order"""
    n, co, ty, tx = acc.shape[:4]
    wy, wx = g.wtiles(h, w)
    a = np.zeros((n, co, 2 * wy, 16 * wx, 6, 6), F32)
    a[:, :, :ty, :tx] = acc
    a = a.reshape(n, co, wy, 2, wx, 16, 6, 6).transpose(0, 2, 4, 1, 3, 5, 6, 7).reshape(n * wy * wx, co, 2, 16, 6, 6).copy()
    grid = min(grid, a.shape[0])
    for t in range(grid, a.shape[0]):
        a[t] += F32(2.0 ** -20) * a[t - grid]
    a = a.reshape(n, wy, wx, co, 2, 16, 6, 6).transpose(0, 3, 1, 4, 2, 5, 6, 7).reshape(n, co, 2 * wy, 16 * wx, 6, 6)
    return a[:, :, :ty, :tx]


def emulate_sums(pre: np.ndarray, k: int, mutant: Optional[str] = None):
    """what the epilogue leaves beside the output, from an fp32 `pre`: part (n, tiles, cout) and the border pieces
    (n, 4, stride, cout) with (p_rows, p_cols), in the layouts DESIGN 4b documents; SUM_MUTANTS exchange two slots"""
    g = Geo(k)
    n, co, h, w = pre.shape
    wy, wx = g.wtiles(h, w)
    pp = np.zeros((n, co, wy * g.toh, wx * g.tow), F32)
    pp[:, :, :h, :w] = pre
    part = pp.reshape(n, co, wy, g.toh, wx, g.tow).sum(axis=(3, 5), dtype=F32).reshape(n, co, wy * wx).transpose(0, 2, 1).copy()
    p_rows, p_cols = wx, 2 * wy
    data = np.zeros((n, 4, max(p_rows, p_cols), co), F32)
    for b, line in enumerate((pre[:, :, 0], pre[:, :, h - 1])):
        lp = np.zeros((n, co, wx * g.tow), F32)
        lp[:, :, :w] = line
        data[:, b, :p_rows] = lp.reshape(n, co, wx, g.tow).sum(axis=3, dtype=F32).transpose(0, 2, 1)
    for b, line in enumerate((pre[:, :, :, 0], pre[:, :, :, w - 1])):
        lp = np.zeros((n, co, p_cols * g.m), F32)
        lp[:, :, :h] = line
        data[:, 2 + b, :p_cols] = lp.reshape(n, co, p_cols, g.m).sum(axis=3, dtype=F32).transpose(0, 2, 1)
    if mutant == "swap_part":
        part[:, [0, 1]] = part[:, [1, 0]]
    elif mutant == "swap_pieces":
        data[:, 2, [0, 1]] = data[:, 2, [1, 0]]
    else:
        assert mutant is None, mutant
    return part, data, p_rows, p_cols


# ------------------------------------------------------------------------------------------ the checks
def _fail(cond, msg):
    if not cond:
        raise AssertionError(msg)


def ratio_uE(out: np.ndarray, ref: np.ndarray, E: np.ndarray) -> float:
    """largest |out - ref| / (u E) over the pixels with E > 0 (plain convolutions: no epilogue terms)"""
    err = np.abs(out.astype(np.float64) - ref)
    ok = E > 0
    return float((err[ok] / (U * E[ok])).max()) if ok.any() else 0.0


def check_local(out: np.ndarray, r: Result, where: Optional[np.ndarray] = None, what: str = "") -> float:
    """|out - ref64| <= bound at EVERY pixel (of `where`); returns the largest err / bound"""
    err = np.abs(out.astype(np.float64) - r.ref)
    good = err <= r.bound          # (False for a NaN)
    if where is not None:
        good = good | ~where
        err = np.where(where, err, 0.0)
    if not good.all():
        i = np.unravel_index(np.argmax(np.where(good, -1.0, np.where(np.isnan(err), np.inf, err / np.maximum(r.bound, 1e-300)))), err.shape)
        _fail(False, f"{what}: {int((~good).sum())} pixels outside the local bound; worst at {tuple(int(v) for v in i)}: out {out[i]!r} "
                     f"ref {r.ref[i]!r} err {err[i]:.3e} bound {r.bound[i]:.3e}")
    pos = r.bound > 0
    return float((err[pos] / r.bound[pos]).max()) if pos.any() else 0.0


def old_global(out: np.ndarray, ref: np.ndarray) -> float:
    """tests/test_hip_ops.py's metric: max|out - ref| / max(1, max|ref|), asserted <= 6e-5 there"""
    return float(np.abs(out.astype(np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


OLD_GLOBAL_TOL = 6e-5


def old_part_ok(part: np.ndarray, pre: np.ndarray) -> bool:
    """tests/test_hip_ops.py's check of the channel sums: after summing over the tile axis, absolute term 5e-3"""
    sums = pre.sum(axis=(2, 3))
    return bool(np.abs(part.astype(np.float64).sum(axis=1) - sums).max() <= 1e-5 * np.abs(sums).max() + 5e-3)


def impulse_pixels(x: np.ndarray) -> List[List[Tuple[int, int]]]:
    """per image: the (y, x) of its nonzero input pixels"""
    nz = np.any(x != 0, axis=1)
    return [[(int(a), int(b)) for a, b in zip(*np.nonzero(nz[i]))] for i in range(x.shape[0])]


def check_impulse(out: np.ndarray, x: np.ndarray, r: Result, k: int, what: str = "") -> int:
    """one-hot inputs, no bias, no activation: exact zero outside the Winograd tiles whose patch holds an impulse (a zero patch
    transforms to zero: arithmetic, not tolerance), the local bound inside them (the flipped weights on the support, the residue
    elsewhere).  Returns the number of exact-zero pixels checked."""
    g = Geo(k)
    n, co, h, w = out.shape
    inside = np.zeros((n, 1, h, w), bool)
    for i, px in enumerate(impulse_pixels(x)):
        inside[i, 0] = g.tile_mask(px, h, w)
    inside = np.broadcast_to(inside, out.shape)
    stray = (out != 0) & ~inside          # (a NaN is != 0 too)
    if stray.any():
        i = tuple(int(v) for v in np.argwhere(stray)[0])
        _fail(False, f"{what}: {int(stray.sum())} nonzero pixels outside every tile that saw an impulse, first at {i}: {out[i]!r}")
    check_local(out, r, inside, what)
    return int((~inside).sum())


def check_nonfinite(out: np.ndarray, bad: Tuple[int, int, int, int], w: np.ndarray, r0: Result, k: int, what: str = "") -> int:
    """one non-finite input pixel bad = (n, ci, y, x); r0: reference and bound of the same input with that pixel set to 0.
    non-finite outputs  >=  the k x k receptive field wherever its weight is nonzero;  <=  the tiles whose patch holds the pixel;
    every other pixel finite and inside the bound.  Returns the number of non-finite outputs."""
    g = Geo(k)
    bn, bc, by, bx = bad
    n, co, h, wd = out.shape
    nf = ~np.isfinite(out)
    tiles = np.zeros(out.shape, bool)
    tiles[bn] = g.tile_mask([(by, bx)], h, wd)[None]
    field_ = np.zeros(out.shape, bool)
    for dy in range(-g.pad, g.pad + 1):
        for dx in range(-g.pad, g.pad + 1):
            y, x = by + dy, bx + dx          # out[y, x] reads in[by, bx] through w[g.pad - dy, g.pad - dx]
            if 0 <= y < h and 0 <= x < wd:
                field_[bn, :, y, x] = w[:, bc, g.pad - dy, g.pad - dx] != 0
    _fail(not (field_ & ~nf).any(), f"{what}: {int((field_ & ~nf).sum())} finite outputs inside the receptive field of the non-finite pixel {bad}")
    _fail(not (nf & ~tiles).any(), f"{what}: {int((nf & ~tiles).sum())} non-finite outputs outside the tiles that hold {bad}, "
                                   f"first at {tuple(int(v) for v in np.argwhere(nf & ~tiles)[0]) if (nf & ~tiles).any() else None}")
    check_local(out, r0, ~tiles, what)
    return int(nf.sum())


def sums64(r: Result, k: int):
    """fp64 channel sums / border pieces of r.pre with their tolerances: the pixels' own bounds added up + depth u sum|pre|"""
    g = Geo(k)
    n, co, h, w = r.pre.shape
    wy, wx = g.wtiles(h, w)

    def blocks(a, ny, by, nx, bx):
        p = np.zeros(a.shape[:2] + (ny * by, nx * bx))
        p[:, :, :a.shape[2], :a.shape[3]] = a
        return p.reshape(n, co, ny, by, nx, bx).sum(axis=(3, 5)).reshape(n, co, ny * nx).transpose(0, 2, 1)

    part = blocks(r.pre, wy, g.toh, wx, g.tow)
    part_tol = blocks(r.bound_pre, wy, g.toh, wx, g.tow) + SUM_DEPTH * U * blocks(np.abs(r.pre), wy, g.toh, wx, g.tow)
    p_rows, p_cols = wx, 2 * wy
    data = np.zeros((n, 4, max(p_rows, p_cols), co))
    tol = np.zeros_like(data)
    for b, sl in enumerate((np.s_[:, :, 0:1, :], np.s_[:, :, h - 1:h, :])):
        data[:, b, :p_rows] = blocks(r.pre[sl], 1, 1, wx, g.tow)
        tol[:, b, :p_rows] = blocks(r.bound_pre[sl], 1, 1, wx, g.tow) + LINE_DEPTH * U * blocks(np.abs(r.pre[sl]), 1, 1, wx, g.tow)
    for b, sl in enumerate((np.s_[:, :, :, 0:1], np.s_[:, :, :, w - 1:w])):
        data[:, 2 + b, :p_cols] = blocks(r.pre[sl], p_cols, g.m, 1, 1)
        tol[:, 2 + b, :p_cols] = blocks(r.bound_pre[sl], p_cols, g.m, 1, 1) + LINE_DEPTH * U * blocks(np.abs(r.pre[sl]), p_cols, g.m, 1, 1)
    return part, part_tol, data, tol, p_rows, p_cols


def check_part(part: np.ndarray, r: Result, k: int, what: str = "") -> float:
    """part[n, tile, co] slot by slot against the fp64 sum of that 8 x 64 (4 x 32) tile's valid pixels; no absolute constant"""
    ref, tol = sums64(r, k)[:2]
    _fail(part.shape == ref.shape, f"{what}: part {part.shape} != {ref.shape}")
    err = np.abs(part.astype(np.float64) - ref)
    good = err <= tol
    _fail(good.all(), f"{what}: {int((~good).sum())} channel-sum slots off, first (n, tile, co) = "
                      f"{tuple(int(v) for v in np.argwhere(~good)[0]) if not good.all() else None}")
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


def check_pieces(data: np.ndarray, p_rows: int, p_cols: int, r: Result, what: str = "") -> float:
    """data[n, border, piece, co], pieces 0 .. p_rows - 1 of borders 0 / 1 (rows 0 / h - 1) and 0 .. p_cols - 1 of borders 2 / 3
    (columns 0 / w - 1), piece by piece; what lies beyond up to the stride is unspecified and not read"""
    _, _, ref, tol, pr, pc = sums64(r, 3)
    _fail((p_rows, p_cols) == (pr, pc), f"{what}: pieces ({p_rows}, {p_cols}) != ({pr}, {pc})")
    worst = 0.0
    for b in range(4):
        cnt = p_rows if b < 2 else p_cols
        err = np.abs(data[:, b, :cnt].astype(np.float64) - ref[:, b, :cnt])
        t = tol[:, b, :cnt]
        good = err <= t
        _fail(good.all(), f"{what}: border {b}: {int((~good).sum())} pieces off, first (n, piece, co) = "
                          f"{tuple(int(v) for v in np.argwhere(~good)[0]) if not good.all() else None}")
        if (t > 0).any():
            worst = max(worst, float((err[t > 0] / t[t > 0]).max()))
    return worst


# ------------------------------------------------------------------------------------------ packed weights
def slot_position(pair: int, lo: int) -> Tuple[int, int]:
    """slot (pair, lo) of the packed form -> transform-domain position (row i, column q): a row's pairs are the columns (1, 2),
    (3, 4), (0, 5)"""
    pp = pair % 3
    return pair // 3, (1 + lo if pp == 0 else 3 + lo if pp == 1 else (5 if lo else 0))


def unpack_u(packed: np.ndarray, cout: int, cin: int):
    """[cot][cin / 4][xi / 2][c][co ^ 16 (c & 1)][xi & 1] -> U (64 cot_n, cin, 6, 6), channels >= cout included (the padding)"""
    cot_n = -(-cout // 64)
    p = packed.reshape(cot_n, cin // 4, 18, 4, 64, 2)
    u = np.empty((cot_n, 64, cin // 4, 4, 6, 6), packed.dtype)
    for pair in range(18):
        for lo in range(2):
            i, q = slot_position(pair, lo)
            for c in range(4):
                col = np.arange(64) ^ ((c & 1) << 4)          # channel co of the block sits in column co ^ 16 (c & 1)
                u[:, :, :, c, i, q] = p[:, :, pair, c, :, lo][:, :, col].transpose(0, 2, 1)
    return u.reshape(cot_n * 64, cin, 6, 6)


# ------------------------------------------------------------------------------------------ the case table
INPUT_KINDS = ("noise", "offset100", "blocks_on", "blocks_off", "quiet_edge")
# the dynamic-range blocks are 12 rows x 16 columns: a Winograd tile's whole 6 x 6 patch fits inside one (quiet tiles exist), the
# row seams y = 12, 24, 36 fall BETWEEN the two tile rows of a workgroup (12, 36) and between workgroups (24), the column seams on
# every fourth tile column and on the 64-pixel workgroup grid; blocks_off moves all of them one pixel up and left
BLOCK_H, BLOCK_W = 12, 16


@dataclass(frozen=True)
class Case:
    id: str
    n: int
    h: int
    w: int
    chans: Tuple[int, ...]
    couts: Tuple[int, ...]
    k: int = 3
    act: Optional[str] = None
    bias: bool = True
    residual: bool = False
    res_scale: bool = False
    shuffle: bool = False
    part: bool = False
    border: bool = False
    via: str = "ops"          # "ops": ops.conv2d; "cabi": straight through eavsr_conv3x3_wino4_f32 (odd chunk counts)
    child: bool = False       # also run in the EAVSR_W4_GRP=0 child (duty-pair schedule with an even chunk count)
    ca: bool = False          # the lab-only fused prologue: the kernel convolves x * ca_scale[n, c] + ca_x

    @property
    def cin(self):
        return sum(self.chans)

    @property
    def cout(self):
        return sum(self.couts)

    @property
    def geo(self):
        return Geo(self.k)

    @property
    def wg_tiles(self):
        wy, wx = self.geo.wtiles(self.h, self.w)
        return self.n * wy * wx

    def rng(self, salt: str = ""):
        return np.random.default_rng(zlib.crc32((self.id + salt).encode()))

    def seams(self, kind: str) -> Tuple[List[int], List[int]]:
        """the rows y and columns x (first pixel of the new block) at which the blocks of a blocks_on / blocks_off frame change"""
        o = 0 if kind == "blocks_on" else 1
        return ([y for y in range(1, self.h) if (y + o) % BLOCK_H == 0], [x for x in range(1, self.w) if (x + o) % BLOCK_W == 0])

    def x(self, kind: str, salt: str = "") -> np.ndarray:
        r = self.rng(kind + salt)
        x = r.standard_normal((self.n, self.cin, self.h, self.w)).astype(F32)
        if kind == "offset100":
            x = (x + F32(100)).astype(F32)
        elif kind in ("blocks_on", "blocks_off"):
            o = 0 if kind == "blocks_on" else 1      # seams on the 4-pixel and 8 x 64 grids | off both by one pixel
            by, bx = (np.arange(self.h) + o) // BLOCK_H, (np.arange(self.w) + o) // BLOCK_W
            cls = (by[None, :, None] + bx[None, None, :] + np.arange(self.n)[:, None, None]) % 3
            x = (x * np.choose(cls, [F32(2.0 ** 12), F32(1), F32(2.0 ** -12)])[:, None]).astype(F32)
        elif kind == "quiet_edge":      # loud inside (x 16), the two outermost rows and columns at 2^-12: what a halo taken from
            ring = np.ones((self.h, self.w), bool)      # the clamped edge instead of zeros would be measured against
            ring[2:-2, 2:-2] = False
            x = np.where(ring, x * F32(2.0 ** -12), x * F32(16)).astype(F32)
        else:
            assert kind == "noise", kind
        return x

    def params(self) -> Dict[str, Optional[np.ndarray]]:
        r = self.rng("params")
        p = dict(w=(r.standard_normal((self.cout, self.cin, self.k, self.k)) / np.sqrt(self.cin * self.k * self.k)).astype(F32),
                 bias=(0.1 * r.standard_normal(self.cout)).astype(F32) if self.bias else None,
                 residual=r.standard_normal((self.n, self.cout, self.h, self.w)).astype(F32) if self.residual else None,
                 res_scale=r.uniform(0.0, 1.0, (self.n, self.cout)).astype(F32) if self.res_scale else None,
                 ca_scale=r.uniform(0.0, 1.0, (self.n, self.cin)).astype(F32) if self.ca else None)
        return p

    def operands(self, kind: str, p) -> Tuple[np.ndarray, Optional[np.ndarray], Conv, np.ndarray]:
        """(x, ca_x, Conv, x32): what the launch takes, the reference / bound of its convolution, what emulate32 takes"""
        x = self.x(kind)
        if not self.ca:
            return x, None, Conv(x, p["w"]), x
        xx = self.x(kind, "_x")
        eff, err = fused_input(x, p["ca_scale"], xx)
        return x, xx, Conv(eff, p["w"], err), (x * p["ca_scale"][:, :, None, None] + xx).astype(F32)

    def epilogue_args(self, p) -> dict:
        return dict(bias=p["bias"], act=self.act, slope=SLOPE, residual=p["residual"], res_scale=p["res_scale"], shuffle=self.shuffle)


def _c(id, n, h, w, chans, couts, **kw):
    return Case(id, n, h, w, tuple(chans), tuple(couts) if isinstance(couts, (tuple, list)) else (couts,), **kw)


CASES: Tuple[Case, ...] = (
    # the remainder sweep: every h mod 8; w mod 64 in 0, 4, 60; w < 64; cout 7, 40, 64, 130
    _c("h8_w64", 2, 8, 64, [8], 64, child=True),
    _c("h9_w68", 1, 9, 68, [8], 7, act="relu", residual=True, part=True, child=True),
    _c("h10_w60", 1, 10, 60, [16], 40, act="lrelu"),
    _c("h11_w4", 3, 11, 4, [8], 8, residual=True),
    _c("h12_w124", 1, 12, 124, [8], 64, act="relu", part=True),
    _c("h13_w128", 1, 13, 128, [8], 130, act="lrelu", residual=True, part=True),
    _c("h14_w132", 1, 14, 132, [24], 40, bias=False),
    _c("h15_w64", 2, 15, 64, [8], 64, act="relu", part=True, border=True),
    _c("border_h9_w132", 2, 9, 132, [8], 64, act="lrelu", residual=True, part=True, border=True),      # pieces: BEFORE the residual
    # frames tall enough for ROW seams of the dynamic-range blocks (y = 12, 24, 36 | 11, 23, 35) beside the column seams
    _c("seams_h40_w68", 2, 40, 68, [8], 64, act="relu", part=True, child=True),
    _c("seams_cabi_h36_w64", 1, 36, 64, [12], 64, via="cabi"),
    _c("seams_f5_h36_w36", 1, 36, 36, [8], [8], k=5),
    # the lab-only fused prologue (conv_wino6_kernel<3, true>): skipped on the product library
    _c("lab_ca", 2, 20, 68, [8], 64, act="relu", ca=True),
    # the instantiations
    _c("cabi_c12", 2, 13, 68, [12], 64, act="relu", via="cabi"),                    # 3 chunks: duty-pair schedule
    _c("cabi_c4_8_8", 1, 9, 64, [4, 8, 8], 64, act="relu", via="cabi"),              # 5 chunks, three sources
    _c("rsc", 2, 12, 68, [16], 64, residual=True, res_scale=True),
    _c("shuffle", 1, 9, 68, [8], 40, act="lrelu", shuffle=True),
    _c("src2", 1, 10, 64, [8, 8], 64, act="relu"),
    _c("src5", 1, 9, 8, [8, 8, 8, 8, 8], 7, act="lrelu", residual=True),
    _c("cin64", 1, 8, 64, [64], 64),
    _c("cin128", 1, 8, 8, [128], 8),
    _c("f5_heads", 1, 7, 36, [8], [8, 16, 48], k=5, act="lrelu", part=True),
    _c("f5_src2", 2, 6, 32, [4, 12], [7], k=5, residual=True),
    # more than 256 workgroup tiles per output-channel block: a persistent workgroup walks two
    _c("rounds", 130, 16, 8, [8], 8, bias=False, child=True),
)


def case(id: str) -> Case:
    return next(c for c in CASES if c.id == id)


# impulse cases (test b): one-hot inputs, no bias, no activation
@dataclass(frozen=True)
class ImpulseCase:
    id: str
    n: int
    h: int
    w: int
    cin: int
    cout: int
    k: int
    images: Optional[Tuple[int, ...]]      # the images that hold an impulse (None: all, image i at pixel i of the row-major walk)
    via: str = "ops"
    child: bool = False
    ca: bool = False          # lab-only fused prologue: the one-hot tensor is r, ca_x is zero, the scales are in [0.5, 1]

    def ca_scale(self) -> np.ndarray:
        return np.random.default_rng(zlib.crc32((self.id + "s").encode())).uniform(0.5, 1.0, (self.n, self.cin)).astype(F32)

    def x(self) -> np.ndarray:
        x = np.zeros((self.n, self.cin, self.h, self.w), F32)
        for j, i in enumerate(range(self.n) if self.images is None else self.images):
            p = i if self.images is None else 37 * j + 5
            x[i, (i + j) % self.cin, (p // self.w) % self.h, p % self.w] = 1
        return x

    def weight(self) -> np.ndarray:
        r = np.random.default_rng(zlib.crc32(self.id.encode()))
        return r.standard_normal((self.cout, self.cin, self.k, self.k)).astype(F32)


IMPULSES: Tuple[ImpulseCase, ...] = (
    ImpulseCase("every_pixel_16x16", 256, 16, 16, 8, 8, 3, None, child=True),       # 512 workgroup tiles: two rounds as well
    ImpulseCase("every_pixel_c12", 256, 16, 16, 12, 64, 3, None, via="cabi"),      # duty-pair schedule
    ImpulseCase("every_pixel_f5", 64, 8, 8, 8, 8, 5, None),
    ImpulseCase("every_pixel_lab_ca", 256, 16, 16, 8, 8, 3, None, ca=True),
    ImpulseCase("rounds", 130, 16, 8, 8, 8, 3, (0, 3, 64, 127, 129), child=True),  # 260 tiles on 256 workgroups
)


def impulse_positions(ic: ImpulseCase) -> Dict[str, set]:
    """the in-patch positions (i, j) the case's impulses take, by the place of the TILE in the image: corner, edge, interior"""
    g = Geo(ic.k)
    ty_n, tx_n = g.tiles(ic.h, ic.w)
    seen = {"corner": set(), "edge": set(), "interior": set()}
    for px in impulse_pixels(ic.x()):
        for y, x in px:
            for ty, tx, i, j in g.tiles_containing(y, x, ic.h, ic.w):
                ey, ex = ty in (0, ty_n - 1), tx in (0, tx_n - 1)
                seen["corner" if ey and ex else "edge" if ey or ex else "interior"].add((i, j))
    return seen


# non-finite cases (test c): (y, x) on a 12 x 68 frame: interior, top edge, bottom-right corner, either side of the workgroup seam
NONFINITE_SHAPE = (2, 8, 12, 68)
NONFINITE_PIXELS = ((5, 6), (0, 9), (11, 67), (7, 63), (8, 64))
