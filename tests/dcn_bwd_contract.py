"""The contract of the sampler-side DCNv2 backward (csrc/dcn_bwd.hip, eavsr_dcnv2_bwd_f32), restated in numpy from the head comment
and the constants of that file -- nothing here imports the library.  Helper of tests/test_dcn_bwd_contract_host.py (CPU) and
tests/test_hip_dcn_bwd_contract.py (GPU); DESIGN.md 4c is the prose.

  geometry   Geo: the 4 x 16 tile, b_tap, the per-wave 13 x 32 window and its test on floor(p), the 16 x 32 unit slab, the unit
             order, grid / per, the slab-slot rule of dcn_bwd_dw_reduce, the gather's tile ranges
  reference  reference(): tests/sampler_domain.dcnv2_backward (positions in fp32, interpolation in fp64) + dweight, and the
             per-element bound c u A from the same backward on absolute values
  emulation  emulate32: the algorithm in fp32, elementwise numpy only (bit-reproducible); MUTANTS: wrong in one way each
  checkers   check_local / check_all (new) and old_ok (what tests/test_hip_backward.py and test_hip_sampler_domain.py assert)
  cases      CASES, OFFSET_FIELDS, VALUE_FIELDS: the shapes and inputs both test files walk
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from tests import sampler_domain as SD

F32 = np.float32
U = 2.0 ** -24                       # unit roundoff of fp32

# ---- constants of csrc/dcn_bwd.hip ---------------------------------------------------------------------------------------------
C, CO, DG, CPG = 64, 64, 8, 8
TH, TW = 4, 16                       # tile: one 16-pixel row per wave, 4 waves
MT = 5                               # 16-row blocks of a group's (tap, channel) rows
WY, WX = 6, 8                        # margins of a wave's dx window around its pixel row
WH, WW = 1 + 2 * WY, TW + 2 * WX     # 13 x 32 cells
UH = TH + 2 * WY                     # rows of a unit's slab: y0 - 6 .. y0 + 9
GRID_MAX = 512
TAG_ROUNDS_MAX = 32                  # 16 pixels x the tap pair of a block share a (cell, channel half) at most

# ---- rounding counts (see reference()) -----------------------------------------------------------------------------------------
C_GEMM = 2 * 64                      # the 64-term dcol GEMM at 2 u per addition inside the matrix instruction
C0_DX, C0_DMASK, C0_DOFF, C0_DW, C0_COL = 17, 13, 11, 8, 8


def b_tap(mt: int, hi: int) -> int:
    """the two taps that share a 16-row block: (0,5) (1,6) (2,7) (3,8) (4, padding = 9)"""
    return mt + 5 if hi else mt


def block_of_tap(tap: int) -> int:
    return tap if tap < MT else tap - MT


@dataclass(frozen=True)
class Geo:
    n: int
    h: int
    w: int

    @property
    def tiles_y(self):
        return -(-self.h // TH)

    @property
    def tiles_x(self):
        return -(-self.w // TW)

    @property
    def per_img(self):
        return self.tiles_x * self.tiles_y

    @property
    def ntiles(self):
        return self.n * self.per_img

    @property
    def total(self):
        return DG * self.ntiles

    @property
    def grid(self):
        return min(self.total, GRID_MAX)

    @property
    def per(self):
        return -(-self.total // self.grid)

    def unit(self, u: int) -> Tuple[int, int, int, int]:
        """(group, image, tile row, tile column): group-major, then image, tile row, tile column"""
        g, t = divmod(u, self.ntiles)
        bn, t = divmod(t, self.per_img)
        ty, tx = divmod(t, self.tiles_x)
        return g, bn, ty, tx

    def unit_of(self, g: int, bn: int, ty: int, tx: int) -> int:
        return g * self.ntiles + (bn * self.tiles_y + ty) * self.tiles_x + tx

    def wg_units(self, b: int) -> range:
        return range(b * self.per, min((b + 1) * self.per, self.total))

    def wg_groups(self, b: int) -> List[int]:
        return sorted({u // self.ntiles for u in self.wg_units(b)})

    def straddlers(self) -> List[int]:
        """workgroups whose units lie in two groups"""
        return [b for b in range(self.grid) if len(self.wg_groups(b)) == 2]

    def slot(self, b: int, g: int) -> int:
        """dcn_bwd_dw_reduce's rule: a workgroup's FIRST group is in slot 0, its second in slot 1"""
        return 0 if (b * self.per) // self.ntiles == g else 1

    def wgs_of_group(self, g: int) -> range:
        return range((g * self.ntiles) // self.per, ((g + 1) * self.ntiles - 1) // self.per + 1)

    def gather_tiles(self, y: int, x: int) -> List[Tuple[int, int]]:
        """the (up to 4 x 2) tiles whose slab holds cell (y, x), in the order dcn_bwd_dx_gather adds them"""
        ty_lo, ty_hi = max((y - WY) >> 2, 0), min((y + WY) >> 2, self.tiles_y - 1)
        tx_lo, tx_hi = max((x - WX) >> 4, 0), min((x + WX) >> 4, self.tiles_x - 1)
        return [(ty_lo + i, tx_lo + j) for i in range(4) for j in range(2) if ty_lo + i <= ty_hi and tx_lo + j <= tx_hi]


def window_coords(fy, fx, gy, x0):
    """(by, bx): floor(p) in the window of the wave whose pixel row is gy, in the tile whose first column is x0"""
    return fy - (gy - WY), fx - (x0 - WX)


def fast_test(by, bx, variant: Optional[str] = None):
    """both corners of either axis inside the 13 x 32 window; variant "b": the off-by-one test of mutant (b)"""
    if variant == "b":
        return (by >= 0) & (by < WH) & (bx >= 0) & (bx < WW)
    return (by >= 0) & (by + 1 < WH) & (bx >= 0) & (bx + 1 < WW)


def sample_geometry(off: np.ndarray, geo: Geo) -> Dict[str, np.ndarray]:
    """per sample (n, 8, 9, h, w): floor(p) (clamped as b_samp clamps it), the gate, window coordinates, fast / atomic path"""
    h, w = geo.h, geo.w
    py, px = SD.dcn_positions(off, DG)
    gate = SD.dcn_gate(py, px, h, w) & np.isfinite(py) & np.isfinite(px)
    fy = np.clip(np.floor(np.where(gate, py, 0)), -2, h).astype(np.int64)
    fx = np.clip(np.floor(np.where(gate, px, 0)), -2, w).astype(np.int64)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    by, bx = window_coords(fy, fx, yy, xx // TW * TW)
    return dict(py=py, px=px, gate=gate, fy=fy, fx=fx, by=by, bx=bx, fast=gate & fast_test(by, bx), yy=yy, xx=xx,
                nonint=(py != np.floor(py)) & (px != np.floor(px)))


def multiplicities(off: np.ndarray, geo: Geo) -> np.ndarray:
    """for every fast sample: how many lanes of its LDS instruction (same unit, wave, tap-pair block) share its (cell, channel half)"""
    s = sample_geometry(off, geo)
    n, h, w = geo.n, geo.h, geo.w
    blk = np.array([block_of_tap(k) for k in range(9)]).reshape(1, 1, 9, 1, 1)
    nn = np.arange(n).reshape(n, 1, 1, 1, 1)
    gg = np.arange(DG).reshape(1, DG, 1, 1, 1)
    key = (((((nn * DG + gg) * h + s["yy"]) * geo.tiles_x + s["xx"] // TW) * MT + blk) * WH + s["by"]) * WW + s["bx"]
    key = np.broadcast_to(key, s["fast"].shape)[s["fast"]]
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return cnt[inv]


def tile_row_coverage(off: np.ndarray, geo: Geo) -> set:
    """{(cell row mod 4, tile row of the contributing unit - first tile row of the gather)} over the in-image corners of fast samples"""
    s = sample_geometry(off, geo)
    out = set()
    ty = np.broadcast_to(s["yy"] // TH, s["fast"].shape)[s["fast"]]
    for d in (0, 1):
        yc = s["fy"][s["fast"]] + d
        ok = (yc >= 0) & (yc < geo.h)
        rel = ty[ok] - np.maximum((yc[ok] - WY) >> 2, 0)
        out |= set(zip((yc[ok] % 4).tolist(), rel.tolist()))
    return out


# ---- reference and bound -------------------------------------------------------------------------------------------------------
@dataclass
class Ref:
    dx: np.ndarray
    doff: np.ndarray
    dmask: np.ndarray
    dw: Optional[np.ndarray]
    b_dx: np.ndarray
    b_doff: np.ndarray
    b_dmask: np.ndarray
    b_dw: Optional[np.ndarray]
    frac_ok: np.ndarray
    cnt: np.ndarray          # (n, 8, h, w): addends that land on each dx cell (per channel)
    col: Optional[np.ndarray] = None
    b_col: Optional[np.ndarray] = None

    def pairs(self):
        return [(k, getattr(self, k), getattr(self, "b_" + k)) for k in ("dx", "doff", "dmask", "dw") if getattr(self, k) is not None]


def gamma(c):
    """Higham's gamma_c = c u / (1 - c u): the first-order count c with its second-order tail"""
    c = np.asarray(c, np.float64)
    return c * U / (1.0 - c * U)


def reference(x, off, mask, wt, dy=None, dcol=None, gemm: bool = True, want_col: bool = False) -> Ref:
    """fp64 reference (tests/sampler_domain.dcnv2_backward; dweight = sum dY col^T) and the per-element bound gamma(c) A.

    A is the same backward on absolute values in fp64: D = |W|^T |dY| for the column gradient, |x|, |mask|, the non-negative corner
    weights, and for doffset the absolute position-derivative terms (|q_far| + |q_near|) x the other axis' weight.  c counts the
    roundings on the longest path to the element, operation by operation in dcn_bwd_kernel (u = 2^-24 each; an fp32 sum of m terms
    in any order is within (m - 1) u sum|t|; additions inside the matrix instruction 2 u each):

      every output   C_GEMM = 2 x 64: the 64-term dcol GEMM (dropped when the column gradient is given, gemm=False)
      dx      m + 17   m = the addends that land on the cell (window read-add-writes, atomics: any order)
                       3 corner weight (1 - lh, 1 - lw, their product), 1 dcol * mask, 1 dv * weight,
                       4 overlap of the four windows into the slab (v += window row), 8 gather (v += slab, eight slots)
      dmask   13       val: 2 (1 - lh, 1 - lw) + 1 (hh * hw) + 1 (* q) + 3 (four-term sum) = 7; 1 dcol * val; 4 gm += over the lane's
                       four channels; 1 cross-lane add
      doffset 11       1 (q3 - q1), 1 (1 - lw), 1 (* hw), 1 (sum of the two terms), 1 dcol * mask, 1 dv * (..), 4 gp += , 1 cross-lane
      dweight m + 8    m = pixels of the batch (one addend each; registers, LDS combine and slab reduce are one sum in some
                       order); val 7, 1 val * mask.  Its C_GEMM term stands for the additions of that sum made INSIDE the matrix
                       instruction at 2 u instead of u: 16 per unit of a workgroup's run, 16 per <= 64 (the host test asserts it)
      columns 8        (dcnv2_im2col: val 7, 1 val * mask)

    No absolute term: A = 0 means the output is exactly +-0."""
    x, off, mask, wt = (np.asarray(a) for a in (x, off, mask, wt))
    n, c, h, w = x.shape
    assert (c, wt.shape) == (C, (CO, C, 3, 3))
    dx, doff, dmask, frac_ok = SD.dcnv2_backward(x, off, mask, wt, dy, DG, dcol=dcol)
    w2 = np.abs(wt.astype(np.float64)).reshape(CO, C * 9)
    if dcol is None:
        D = np.einsum("ok,nop->nkp", w2, np.abs(np.asarray(dy, np.float64)).reshape(n, CO, h * w))
    else:
        D = np.abs(np.asarray(dcol, np.float64)).reshape(n, C * 9, h * w)
    D = D.reshape(n, DG, CPG, 9, h, w)
    py, px = SD.dcn_positions(off, DG)
    gate = SD.dcn_gate(py, px, h, w) & np.isfinite(py) & np.isfinite(px)
    am = np.abs(mask.astype(np.float64)).reshape(n, DG, 9, h, w)
    ax = np.abs(x.astype(np.float64)).reshape(n, DG, CPG, h, w)
    nidx = np.arange(n).reshape(n, 1, 1, 1, 1)
    gidx = np.arange(DG).reshape(1, DG, 1, 1, 1)
    a_dx = np.zeros((n, DG, CPG, h * w))
    cnt = np.zeros((n, DG, h * w))
    a_dm, a_py, a_px = (np.zeros((n, DG, 9, h, w)) for _ in range(3))
    plane = (nidx * DG + gidx) * (h * w)
    for cy, cx, wgt, ins, (sy, sx, wy, wx) in SD._corners(py, px, h, w, gate):
        flat = (plane + cy * w + cx).ravel()
        cnt += np.bincount(flat, weights=ins.ravel().astype(np.float64), minlength=n * DG * h * w).reshape(n, DG, h * w)
        for cc in range(CPG):
            v = np.where(ins, ax[nidx, gidx, cc, cy, cx], 0.0)
            d = D[:, :, cc]
            a_dm += d * wgt * v
            a_py += d * am * v * np.where(gate, wx, 0.0)
            a_px += d * am * v * np.where(gate, wy, 0.0)
            a_dx[:, :, cc] += np.bincount(flat, weights=(d * am * wgt).ravel(), minlength=n * DG * h * w).reshape(n, DG, h * w)
    g0 = C_GEMM if gemm else 0
    cnt = cnt.reshape(n, DG, h, w)
    b_dx = (gamma(g0 + C0_DX + cnt)[:, :, None] * a_dx.reshape(n, DG, CPG, h, w)).reshape(n, C, h, w)
    b_doff = gamma(g0 + C0_DOFF) * np.stack([a_py, a_px], 3).reshape(n, DG * 18, h, w)
    b_dm = gamma(g0 + C0_DMASK) * a_dm.reshape(n, DG * 9, h, w)
    dw = b_dw = col = b_col = None
    if dy is not None or want_col:
        col = SD.dcn_columns(x, off, mask, DG)
        acol = SD.dcn_columns(np.abs(x), off, np.abs(mask), DG)
        b_col = gamma(C0_COL) * acol
    if dy is not None:
        dy64 = np.asarray(dy, np.float64).reshape(n, CO, h * w)
        dw = np.einsum("nop,nkp->ok", dy64, col.reshape(n, C * 9, h * w)).reshape(CO, C, 3, 3)
        a_dw = np.einsum("nop,nkp->ok", np.abs(dy64), acol.reshape(n, C * 9, h * w)).reshape(CO, C, 3, 3)
        b_dw = gamma(C_GEMM + C0_DW + n * h * w) * a_dw
    return Ref(dx, doff, dmask, dw, b_dx, b_doff, b_dm, b_dw, frac_ok, cnt, col, b_col)


# ---- the checks ----------------------------------------------------------------------------------------------------------------
def _fail(cond, msg):
    if not cond:
        raise AssertionError(msg)


def check_local(out: np.ndarray, ref: np.ndarray, bound: np.ndarray, what: str = "") -> float:
    """|out - ref| <= bound at EVERY element (bound 0: the element is exactly +-0); returns the largest err / bound"""
    out = np.asarray(out)
    _fail(out.shape == ref.shape, f"{what}: shape {out.shape} != {ref.shape}")
    err = np.abs(out.astype(np.float64) - ref)
    good = err <= bound          # (False for a NaN)
    if not good.all():
        score = np.where(good, -1.0, np.where(np.isnan(err), np.inf, err / np.maximum(bound, 1e-300)))
        i = np.unravel_index(np.argmax(score), err.shape)
        _fail(False, f"{what}: {int((~good).sum())} of {good.size} elements outside the local bound ({int((~good & (bound == 0)).sum())} of them "
                     f"where the bound is exact zero); worst at {tuple(int(v) for v in i)}: out {out[i]!r} ref {ref[i]!r} err {err[i]:.3e} "
                     f"bound {bound[i]:.3e}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def check_all(got: Dict[str, np.ndarray], r: Ref, what: str = "") -> Dict[str, float]:
    """dx, doff, dmask, dw of `got` (a missing or None entry is not checked) against r; no element is excluded (frac_ok all true)"""
    _fail(bool(r.frac_ok.all()), f"{what}: {int((~r.frac_ok).sum())} doffset entries at integer positions")
    return {k: check_local(got[k], ref, b, f"{what} {k}") for k, ref, b in r.pairs() if got.get(k) is not None}


OLD_TOL = {"dx": 1e-4, "doff": 1e-4, "dmask": 1e-4, "dw": 2e-5}


def old_metric(out: np.ndarray, ref: np.ndarray) -> float:
    """tests/test_hip_backward.py / test_hip_sampler_domain.py: max|out - ref| / max(1, max|ref|), asserted <= 1e-4 (2e-5 for
    dweight against the column path)"""
    return float(np.abs(np.asarray(out, np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


def old_ok(got: Dict[str, np.ndarray], r: Ref) -> bool:
    return all(old_metric(got[k], ref) <= OLD_TOL[k] for k, ref, _ in r.pairs() if got.get(k) is not None)


def new_ok(got, r: Ref) -> bool:
    try:
        check_all(got, r)
        return True
    except AssertionError:
        return False


# ---- the fp32 emulation and its mutants ----------------------------------------------------------------------------------------
MUTANTS = ("a", "b", "c", "d", "e", "f", "f1", "g", "h")
MUTANT_DOC = {
    "a": "the tag loop gives up after 16 rounds: lanes 17 .. 32 of a cell lose their addend",
    "b": "the fast test is by < 13, bx < 32: far corners land on the next window row's first cells / the next wave's window",
    "c": "window row 12 of wave 3 is not re-zeroed between the units of a workgroup",
    "d": "the gather reads three tile rows, not four",
    "e": "the two slab slots of a straddling workgroup are exchanged",
    "f": "the flush at a group boundary scales the dW accumulators by 2^-20 instead of zeroing them",
    "f1": "a workgroup's second unit of the same group starts its dW accumulators from 2^-20 x the first's, not 1 x",
    "g": "doffset of a gate-invalid sample is what its clamped corners give, not 0",
    "h": "need_dx=False also skips dmask",
}
_WCELLS = 4 * WH * WW          # window cells of a workgroup
_WPITCH = _WCELLS + 64         # + where mutant (b)'s overflow past wave 3's window lands (read by nobody)


def _rank(keys: np.ndarray) -> np.ndarray:
    """rank of every entry among the entries with the same key, in array order"""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    first = np.r_[True, sk[1:] != sk[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(sk.size), 0))
    rank = np.empty(sk.size, np.int64)
    rank[order] = np.arange(sk.size) - start
    return rank


def _add_rounds(target: np.ndarray, idx: np.ndarray, vals: np.ndarray, max_rounds: Optional[int] = None) -> None:
    """target[idx] += vals with repeated indices served one per round (each round is one elementwise fp32 add)"""
    if idx.size == 0:
        return
    rank = _rank(idx)
    for r in range(int(rank.max()) + 1 if max_rounds is None else min(int(rank.max()) + 1, max_rounds)):
        s = rank == r
        target[idx[s]] = target[idx[s]] + vals[s]


def _seq_sum(a: np.ndarray) -> np.ndarray:
    """((a0 + a1) + a2) + a3 over the last axis"""
    v = a[..., 0]
    for i in range(1, a.shape[-1]):
        v = v + a[..., i]
    return v


def emulate32(x, off, mask, wt, dy, need_dx: bool = True, mutant: Optional[str] = None, accumulate_into: Optional[np.ndarray] = None):
    """dict(dx, doff, dmask, dw): the launch chain of eavsr_dcnv2_bwd_f32 in fp32, every operation an elementwise numpy one -- dcol
    accumulated over co, per-lane contributions, per-wave windows with tag rounds, overlap into unit slabs, gather, dW accumulators
    per (workgroup, wave) flushed per group into slot 0 / 1 and reduced by the slot rule.  Workgroups run side by side, a
    workgroup's units one after the other.  `mutant` makes it wrong in one way (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS, mutant
    x, off, mask, wt, dy = (np.ascontiguousarray(a, F32) for a in (x, off, mask, wt, dy))
    n, _, h, w = x.shape
    geo = Geo(n, h, w)
    hw = h * w
    xil = np.ascontiguousarray(x.reshape(n, DG, CPG, h, w).transpose(0, 1, 3, 4, 2))
    o = off.reshape(n, DG, 9, 2, h, w)
    m = mask.reshape(n, DG, 9, h, w)
    wg = np.ascontiguousarray(wt.reshape(CO, DG, CPG, 9).transpose(1, 0, 3, 2))      # [g][co][tap][c]
    dxil = np.zeros((n * DG * hw, CPG), F32)
    doff = np.zeros((n, DG, 9, 2, h, w), F32)
    dmask = np.zeros((n, DG, 9, h, w), F32)
    dxs = np.zeros((geo.total, UH, WW, CPG), F32)
    slabs = np.zeros((geo.grid, 2, CO, 9, CPG), F32)
    acc = np.zeros((geo.grid, 4, CO, 9, CPG), F32)
    win = np.zeros((geo.grid * _WPITCH, CPG), F32)
    cur_g = np.full(geo.grid, -1)
    slot = np.zeros(geo.grid, np.int64)
    wave = np.arange(4).reshape(1, 4, 1)
    l15 = np.arange(16).reshape(1, 1, 16)
    ky = (np.arange(9) // 3 - 1)
    kx = (np.arange(9) % 3 - 1)
    one = F32(1)

    def flush(bs):
        v = acc[bs, 0]
        for wv in range(1, 4):
            v = v + acc[bs, wv]
        slabs[bs, slot[bs]] = v
        acc[bs] = acc[bs] * F32(2.0 ** -20) if mutant == "f" else F32(0)

    for j in range(geo.per):
        b_all = np.arange(geo.grid)
        u_all = b_all * geo.per + j
        live = u_all < np.minimum((b_all + 1) * geo.per, geo.total)
        bb, ub = b_all[live], u_all[live]
        g = ub // geo.ntiles
        change = (g != cur_g[bb]) & (cur_g[bb] >= 0)
        if mutant == "f1":
            same = bb[g == cur_g[bb]]
            acc[same] = acc[same] * F32(2.0 ** -20)
        if change.any():
            flush(bb[change])
            slot[bb[change]] = 1
        cur_g[bb] = g
        t = ub - g * geo.ntiles
        bn = t // geo.per_img
        t = t - bn * geo.per_img
        ty, tx = t // geo.tiles_x, t % geo.tiles_x
        y0, x0 = (ty * TH).reshape(-1, 1, 1), (tx * TW).reshape(-1, 1, 1)
        gy, gx = np.broadcast_arrays(y0 + wave, x0 + l15)                      # (units, 4, 16)
        pvalid = (gy < h) & (gx < w)
        yy, xx = np.where(pvalid, gy, 0), np.where(pvalid, gx, 0)
        b3, g3 = bn.reshape(-1, 1, 1), g.reshape(-1, 1, 1)
        dyp = np.where(pvalid[..., None], dy[b3, :, yy, xx], F32(0))           # (units, 4, 16, 64)
        # dcol[unit, wave, pixel, tap, c] = sum over co, in order, in fp32
        dcol = np.zeros(gy.shape + (9, CPG), F32)
        wgu = wg[g]                                                            # (units, 64, 9, 8)
        for co in range(CO):
            dcol = dcol + wgu[:, co][:, None, None] * dyp[..., co][..., None, None]
        # the sampler (b_samp)
        oy, ox = o[b3, g3, :, 0, yy, xx], o[b3, g3, :, 1, yy, xx]              # (units, 4, 16, 9)
        mm = m[b3, g3, :, yy, xx]
        py = (gy[..., None] + ky).astype(F32) + oy
        px = (gx[..., None] + kx).astype(F32) + ox
        py = np.minimum(np.maximum(py, F32(-2)), F32(h + 1))
        px = np.minimum(np.maximum(px, F32(-2)), F32(w + 1))
        in_ = (py > -1) & (px > -1) & (py < h) & (px < w)
        fy0, fx0 = np.floor(py), np.floor(px)
        lh, lw = py - fy0, px - fx0
        hh, hw_ = one - lh, one - lw
        hl = np.clip(fy0, -2, h).astype(np.int64)
        wl = np.clip(fx0, -2, w).astype(np.int64)
        t_ok, b_ok, l_ok, r_ok = hl >= 0, hl + 1 <= h - 1, wl >= 0, wl + 1 <= w - 1
        vs = [in_ & t_ok & l_ok, in_ & t_ok & r_ok, in_ & b_ok & l_ok, in_ & b_ok & r_ok]
        wraw = [hh * hw_, hh * lw, lh * hw_, lh * lw]
        ws = [np.where(v, p, F32(0)) for v, p in zip(vs, wraw)]
        cy = [np.clip(hl, 0, h - 1), np.clip(hl, 0, h - 1), np.clip(hl + 1, 0, h - 1), np.clip(hl + 1, 0, h - 1)]
        cx = [np.clip(wl, 0, w - 1), np.clip(wl + 1, 0, w - 1), np.clip(wl, 0, w - 1), np.clip(wl + 1, 0, w - 1)]
        b4, g4 = b3[..., None], g3[..., None]
        raw = [xil[b4, g4, cy[k], cx[k]] for k in range(4)]                    # (units, 4, 16, 9, 8)
        q = [np.where(vs[k][..., None], raw[k], F32(0)) for k in range(4)]
        val = ((wraw[0][..., None] * q[0] + wraw[1][..., None] * q[1]) + wraw[2][..., None] * q[2]) + wraw[3][..., None] * q[3]
        tv = np.broadcast_to(pvalid[..., None], in_.shape)
        col = np.where(tv[..., None], val * mm[..., None], F32(0))

        def halves(p):      # the lane's four channels in order, then the cross-lane add
            return _seq_sum(p[..., :4]) + _seq_sum(p[..., 4:])

        dv = dcol * mm[..., None]
        gm = halves(dcol * val)
        qd = raw if mutant == "g" else q
        gpy = halves(dv * ((qd[2] - qd[0]) * hw_[..., None] + (qd[3] - qd[1]) * lw[..., None]))
        gpx = halves(dv * ((qd[1] - qd[0]) * hh[..., None] + (qd[3] - qd[2]) * lh[..., None]))
        if mutant != "g":
            gpy, gpx = np.where(in_, gpy, F32(0)), np.where(in_, gpx, F32(0))
        kk = np.broadcast_to(np.arange(9), in_.shape)
        sel = (np.broadcast_to(b4, in_.shape)[tv], np.broadcast_to(g4, in_.shape)[tv], kk[tv])
        pix = (np.broadcast_to(yy[..., None], in_.shape)[tv], np.broadcast_to(xx[..., None], in_.shape)[tv])
        doff[sel + (0,) + pix] = gpy[tv]
        doff[sel + (1,) + pix] = gpx[tv]
        if not (mutant == "h" and not need_dx):
            dmask[sel + pix] = gm[tv]
        # dx: windows (tag rounds) or atomics
        if need_dx:
            part = tv & in_
            by, bx = window_coords(hl, wl, gy[..., None], x0[..., None])
            fast = part & fast_test(by, bx, "b" if mutant == "b" else None)
            plane = (b4 * DG + g4) * hw
            dxc = [dv * ws[k][..., None] for k in range(4)]
            for k in range(4):
                s = part & ~fast & vs[k]
                _add_rounds(dxil, (plane + cy[k] * w + cx[k])[s], dxc[k][s])
            wbase = bb.reshape(-1, 1, 1, 1) * _WPITCH + wave[..., None] * (WH * WW)
            cell = wbase + by * WW + bx
            for mt in range(MT):
                taps = [mt, mt + 5] if mt < 4 else [mt]
                f = fast[..., taps]
                if not f.any():
                    continue
                cl = cell[..., taps][f]
                rank = _rank(cl)
                rounds = int(rank.max()) + 1
                assert rounds <= TAG_ROUNDS_MAX, rounds
                if mutant == "a":
                    rounds = min(rounds, 16)
                vals = [dxc[k][..., taps, :][f] for k in range(4)]
                for r in range(rounds):
                    s = rank == r
                    for k in range(4):
                        i = cl[s] + (k >> 1) * WW + (k & 1)
                        win[i] = win[i] + vals[k][s]
            # the unit's slab: the four windows added where they overlap; the windows are zero again
            wv4 = win.reshape(geo.grid, _WPITCH, CPG)[bb]
            w4 = wv4[:, :_WCELLS].reshape(-1, 4, WH, WW, CPG)
            for r in range(UH):
                v = np.zeros((bb.size, WW, CPG), F32)
                for wv in range(4):
                    if 0 <= r - wv < WH:
                        v = v + w4[:, wv, r - wv]
                dxs[ub, r] = v
            keep = w4[:, 3, WH - 1].copy()
            wv4[:] = F32(0)
            if mutant == "c":
                wv4[:, _WCELLS - WW:_WCELLS] = keep
            win.reshape(geo.grid, _WPITCH, CPG)[bb] = wv4
        # dW_g += dY . col^T over the wave's 16 pixels, in pixel order
        a = acc[bb]
        for p in range(16):
            a = a + dyp[:, :, p, :, None, None] * col[:, :, p, None, :, :]
        acc[bb] = a
    flush(np.nonzero(cur_g >= 0)[0])
    # dcn_bwd_dw_reduce: eight slabs at a time, in workgroup order
    dw = np.zeros((CO, DG, CPG, 9), F32)
    two_groups = set(geo.straddlers())
    for g in range(DG):
        bs = list(geo.wgs_of_group(g))
        v0, v1 = np.zeros((CO, 9, CPG), F32), np.zeros((CO, 9, CPG), F32)
        for i in range(0, len(bs), 8):
            tt = []
            for jj in range(8):
                if i + jj < len(bs):
                    b = bs[i + jj]
                    s = geo.slot(b, g)
                    if mutant == "e" and b in two_groups:
                        s = 1 - s
                    tt.append(slabs[b, s])
                else:
                    tt.append(np.zeros((CO, 9, CPG), F32))
            v0 = v0 + ((tt[0] + tt[1]) + (tt[2] + tt[3]))
            v1 = v1 + ((tt[4] + tt[5]) + (tt[6] + tt[7]))
        dw[:, g] = (v0 + v1).transpose(0, 2, 1)
    dw = dw.reshape(CO, C, 3, 3)
    if accumulate_into is not None:
        dw = np.asarray(accumulate_into, F32) + dw
    out = dict(dx=None, doff=doff.reshape(n, DG * 18, h, w), dmask=dmask.reshape(n, DG * 9, h, w), dw=dw)
    if need_dx:
        # dcn_bwd_dx_gather: per cell the (up to 4 x 2) slabs that cover it, in unit order
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        ty_lo, ty_hi = np.maximum((ys - WY) >> 2, 0), np.minimum((ys + WY) >> 2, geo.tiles_y - 1)
        tx_lo, tx_hi = np.maximum((xs - WX) >> 4, 0), np.minimum((xs + WX) >> 4, geo.tiles_x - 1)
        v = dxil.reshape(n, DG, h, w, CPG)
        nn = np.arange(n).reshape(n, 1, 1, 1)
        gg = np.arange(DG).reshape(1, DG, 1, 1)
        for i in range(3 if mutant == "d" else 4):
            for jj in range(2):
                ty, tx = ty_lo + i, tx_lo + jj
                ok = (ty <= ty_hi) & (tx <= tx_hi)
                tyc, txc = np.where(ok, ty, 0), np.where(ok, tx, 0)
                u = gg * geo.ntiles + (nn * geo.tiles_y + tyc) * geo.tiles_x + txc
                r, c = np.where(ok, ys - TH * tyc + WY, 0), np.where(ok, xs - TW * txc + WX, 0)
                v = v + np.where(ok[None, None, :, :, None], dxs[u, r, c], F32(0))
        out["dx"] = np.ascontiguousarray(v.transpose(0, 1, 4, 2, 3)).reshape(n, C, h, w)
    return out


# ---- the case table ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    n: int
    h: int
    w: int

    @property
    def geo(self):
        return Geo(self.n, self.h, self.w)


CASES: Tuple[Case, ...] = (
    Case("per1_ragged", 2, 7, 21),        # per = 1, ragged last tile row and column, waves without pixels
    Case("per2_straddle", 1, 20, 208),    # 65 tiles, per = 2: every odd group boundary falls inside a workgroup
    Case("per2_ragged", 1, 18, 201),      # the same counts with ragged edges
    Case("per2_images", 5, 7, 97),        # 70 tiles, boundaries aligned; 14 tiles per image: no workgroup of two mixes images
    Case("per2_two_images", 3, 20, 80),   # 25 tiles per image, 75 tiles, per = 2: workgroups 12, 49, .. hold the last tile of one image
                                          # and the first of the next; workgroup 37 straddles a group boundary from image 2 to image 0
    Case("per3_splits", 1, 28, 304),      # 133 tiles, per = 3, 1 + 2 and 2 + 1 straddles, idle trailing workgroups
)
OFFSET_FIELDS = ("noise", "seams", "converge", "far")
VALUE_FIELDS = ("noise", "blocks", "masked")
FRACS = (0.25, 0.5, 0.75)
SEAM_ROWS = (-1, 0, WH - 2, WH - 1)
SEAM_COLS = (-1, 0, WW - 2, WW - 1)
CONVERGE = (32, 2, 3, 16, 17, "chain")


def case(id: str) -> Case:
    return next(c for c in CASES if c.id == id)


def _rng(*key) -> np.random.RandomState:
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _noise_offsets(cs: Case, salt: str) -> np.ndarray:
    """sigma = 1 offsets on the quarter grid, never an integer: every fraction of a position is 0.25, 0.5 or 0.75"""
    q = np.rint(_rng(cs.id, salt).standard_normal((cs.n, DG, 9, 2, cs.h, cs.w)) * 4)
    q = np.where(q % 4 == 0, q + 1, q)
    return (q / 4).astype(F32)


def _set(o: np.ndarray, bn, g, k, y, x, ty_, tx_) -> None:
    """the sample (bn, g, k) of pixel (y, x) goes to position (ty_, tx_)"""
    o[bn, g, k, 0, y, x] = F32(ty_) - F32(y - 1 + k // 3)
    o[bn, g, k, 1, y, x] = F32(tx_) - F32(x - 1 + k % 3)


def seam_plan(cs: Case) -> List[dict]:
    """for every tile and wave row: one sample with floor(p) at each of the window rows -1, 0, 11, 12 and columns -1, 0, 30, 31
    whose two corners on that axis lie inside the image; round robin over taps and groups"""
    plan, i = [], 0
    geo = cs.geo
    for bn in range(cs.n):
        for ty in range(geo.tiles_y):
            for tx in range(geo.tiles_x):
                x0 = tx * TW
                cols = min(TW, cs.w - x0)
                for wv in range(TH):
                    gy = ty * TH + wv
                    if gy >= cs.h:
                        continue
                    for axis, slots in ((0, SEAM_ROWS), (1, SEAM_COLS)):
                        for s in slots:
                            fl = (gy - WY + s) if axis == 0 else (x0 - WX + s)
                            if not 0 <= fl <= (cs.h, cs.w)[axis] - 2:
                                continue
                            plan.append(dict(bn=bn, ty=ty, tx=tx, wave=wv, axis=axis, slot=s, fl=fl, frac=FRACS[i % 3], y=gy,
                                             x=x0 + (5 * i) % cols, k=i % 9, g=(i // 9) % DG))
                            i += 1
    return plan


def converge_plan(cs: Case) -> List[dict]:
    """(tile, wave, group, tap-pair block, kind): in full tiles (16 columns, a target row inside the image three rows off the
    pixel row) -- the first, the middle and the last of them -- one block per kind of CONVERGE"""
    geo = cs.geo
    full = [(bn, ty, tx) for bn in range(cs.n) for ty in range(geo.tiles_y) for tx in range(geo.tiles_x) if tx * TW + TW <= cs.w]
    picks = [full[0], full[len(full) // 2], full[-1]]
    plan, i = [], 0
    for bn, ty, tx in picks:
        for wv in range(TH):
            gy = ty * TH + wv
            if gy >= cs.h:
                continue
            fy = gy + 3 if gy + 4 <= cs.h - 1 else gy - 3
            if not 0 <= fy <= cs.h - 2:
                continue
            for kind in CONVERGE:
                mt = i % 4
                plan.append(dict(bn=bn, ty=ty, tx=tx, wave=wv, g=(3 * i + wv) % DG, mt=mt, kind=kind, fy=fy, fx=tx * TW + 4))
                i += 1
    return plan


def offsets(cs: Case, field: str) -> np.ndarray:
    """(n, 144, h, w) fp32, built by placement over the quarter-grid noise"""
    assert field in OFFSET_FIELDS, field
    o = _noise_offsets(cs, "off")
    n, h, w = cs.n, cs.h, cs.w
    if field == "seams":
        for p in seam_plan(cs):
            tgt = [p["y"] + 0.25, p["x"] + 0.25]
            tgt[p["axis"]] = p["fl"] + p["frac"]
            _set(o, p["bn"], p["g"], p["k"], p["y"], p["x"], *tgt)
    elif field == "converge":
        for p in converge_plan(cs):
            x0, gy = p["tx"] * TW, p["ty"] * TH + p["wave"]
            taps = (p["mt"], p["mt"] + 5)
            for k in taps:      # the block's other lanes: each at its own cell (taps t, t + 5 are a filter row apart), rows gy - 1 .. gy + 1
                o[p["bn"], p["g"], k, :, gy, x0:x0 + TW] = F32(0.25)
            lanes = [(l, k) for k in taps for l in range(TW)]      # lane order: the low tap's 16 pixels, then the high tap's
            if p["kind"] == "chain":      # neighbours one cell apart: corner k + 1 of one lane is corner k of the next
                for l in range(TW):
                    _set(o, p["bn"], p["g"], taps[0], gy, x0 + l, p["fy"] + 0.5, x0 - 1 + l + 0.75)
            else:
                for l, k in lanes[:p["kind"]]:
                    _set(o, p["bn"], p["g"], k, gy, x0 + l, p["fy"] + 0.5, p["fx"] + 0.25)
    elif field == "far":
        idx = np.arange(n * DG * 9 * h * w).reshape(n, DG, 9, h, w)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        sel = idx % 4 == 0
        kind = (idx // 4) % 4      # 0: rows away, 1: columns away, 2: the slab's last row (wave 3), 3: the slab's rows from the tile below
        dist_y, dist_x = 8 + (idx // 16) % 5, 32 + (idx // 16) % 17      # 2 - 3 tiles
        up = np.where(yy - dist_y >= 0, yy - dist_y, np.where(yy + dist_y <= h - 2, yy + dist_y, np.where(yy >= h // 2, 0, h - 2)))
        left = np.where(xx - dist_x >= 0, xx - dist_x, np.where(xx + dist_x <= w - 2, xx + dist_x, np.where(xx >= w // 2, 0, w - 2)))
        ty_ = np.where(kind == 0, up, yy).astype(np.float64)
        tx_ = np.where(kind == 1, left, xx).astype(np.float64)
        # wave 3's floor row gy + 5 (window row 11: its lower corner is row 15 of the slab, at y = 1 mod 4 of the tile two rows down);
        # wave 0's floor row gy - 4 (its lower corner at y = 1 mod 4 is covered by four tile rows, this tile being the last of them)
        ty_ = np.where((kind == 2) & (yy % 4 == 3) & (yy + 6 <= h - 1), yy + 5, ty_)
        ty_ = np.where((kind == 3) & (yy % 4 == 0) & (yy - 4 >= 0), yy - 4, ty_)
        ky = (np.arange(9) // 3 - 1).reshape(1, 1, 9, 1, 1)
        kx = (np.arange(9) % 3 - 1).reshape(1, 1, 9, 1, 1)
        fr = np.array(FRACS)[(idx // 7) % 3]
        oy = (ty_ + fr - (yy + ky)).astype(F32)
        ox = (tx_ + 0.25 - (xx + kx)).astype(F32)
        o[:, :, :, 0] = np.where(sel, oy, o[:, :, :, 0])
        o[:, :, :, 1] = np.where(sel, ox, o[:, :, :, 1])
    return np.ascontiguousarray(o.reshape(n, DG * 18, h, w))


def masked_rects(cs: Case) -> List[Tuple[int, int, int, int, float]]:
    """(y0, y1, x0, x1, gain): where the `masked` dy is not zero -- the image's first and last tiles (the units of the workgroups
    that straddle a group boundary) at 2^-16, a rectangle off the tile grid a quarter of the way across at full scale"""
    h, w = cs.h, cs.w
    return [(0, min(3, h), 3, min(20, w), 2.0 ** -16), (max(h - 3, 0), h, max(w - 19, 0), w - 1, 2.0 ** -16),
            (h // 2 - 2, h // 2 + 3, max(w // 4 - 9, 0), w // 4 + 10, 1.0)]


MASKED_ZERO_GROUPS = (1, 4)      # `masked`: the modulation mask of these deformable groups is exactly 0


def values(cs: Case, field: str) -> Dict[str, np.ndarray]:
    """x, mask, wt, dy (fp32)"""
    assert field in VALUE_FIELDS, field
    n, h, w = cs.n, cs.h, cs.w
    r = _rng(cs.id, "values")
    x = r.standard_normal((n, C, h, w)).astype(F32)
    mask = r.uniform(0.1, 1.0, (n, DG * 9, h, w)).astype(F32)
    wt = (r.standard_normal((CO, C, 3, 3)) / 24.0).astype(F32)
    dy = r.standard_normal((n, CO, h, w)).astype(F32)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    gains = np.array([2.0 ** 12, 1.0, 2.0 ** -12], F32)
    if field == "blocks":      # 6 rows x 24 columns: off the 4 x 16 grid in both directions; the transposed pattern on x
        nn = np.arange(n).reshape(n, 1, 1)
        dy = dy * gains[(yy // 6 + xx // 24 + nn) % 3][:, None]
        x = x * gains[(yy // 24 + xx // 6 + nn) % 3][:, None]
    elif field == "masked":
        gain = np.zeros((h, w), F32)
        for y0, y1, x0, x1, gn in masked_rects(cs):
            gain[y0:y1, x0:x1] = gn
        dy = dy * gain
        for g in MASKED_ZERO_GROUPS:
            mask[:, 9 * g:9 * g + 9] = 0
    return dict(x=x.astype(F32), mask=mask, wt=wt, dy=dy.astype(F32))


@functools.lru_cache(maxsize=None)
def inputs(case_id: str, ofield: str, vfield: str):
    """(dict of read-only fp32 inputs, Ref): computed once per combination"""
    cs = case(case_id)
    v = values(cs, vfield)
    v["off"] = offsets(cs, ofield)
    for a in v.values():
        a.setflags(write=False)
    return v, reference(v["x"], v["off"], v["mask"], v["wt"], v["dy"])
