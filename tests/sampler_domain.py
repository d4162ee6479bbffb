"""The sampler domain ("Sampler domain"): the table of sampling positions at which a bilinear sampler can go wrong
-- image edges, the seams of the DCNv2 kernels' LDS windows, wild and non-finite offsets -- builders that scatter the table over
(pixel, tap, group), and float64 numpy references of the contract.  No GPU, no torch: numpy only.

A POSITION is what the kernel's own documented fp32 formula produces; the references recompute it in numpy float32, step by step,
and interpolate in float64.

    DCNv2        p = fl(fl(pixel + (tap - 1)) + offset)            (heads mode: offset = fl(fl(fl(T0 ry + T1 rx) - ry) + t))
    flow_warp    g = fl(pixel + flow); n = fl(fl(fl(2 g) / max(size - 1, 1)) - 1); p = fl(fl(fl(n + 1) / 2) * (size - 1))
    pwc_backwarp g = fl(fl(-1 + fl((2 pixel + 1) / size)) + fl(fl(flow fmul) / fl((size - 1) / 2)));  p = ((g + 1) size - 1) / 2,
                 the product and the subtraction rounded separately or fused: both are computed, either is accepted per pixel

The contract: a finite position contributes weight x value per corner inside the image (DCNv2: only if -1 < p < size on both axes;
`border` clamps the position first); a non-finite position contributes exactly 0 (DCNv2, flow_warp `zeros`, pwc_backwarp, whose mask is
0 there); a gate-invalid sample adds exactly 0 to dx and has doffset / dflow / dmask exactly 0."""
from __future__ import annotations

import numpy as np

F32 = np.float32
INF, NAN = float("inf"), float("nan")
E10 = 2.0 ** -10

# ---- the table.  An entry is (kind, a, b): kind "pos" -> the TARGET position a + b * size (the offset is target - base), kind "off"
# -> the offset / flow value a itself (the position is base + a in fp32)
EDGE = [("pos", -1 - E10, 0), ("pos", -1.0, 0), ("pos", -1 + E10, 0), ("pos", -0.5, 0), ("pos", -0.0, 0), ("pos", 0.0, 0),
        ("pos", -1 - E10, 1), ("pos", -1.0, 1), ("pos", -1 + E10, 1), ("pos", -0.5, 1), ("pos", 0.0, 1)]
WILD_FINITE = [("pos", 4.0, 1), ("pos", -4.0, -1)] + [("off", s * v, 0) for v in (2.0 ** 16, 2.0 ** 24, 2.0 ** 31 - 128, 2.0 ** 31, 2.0 ** 32, 3e38)
                                                      for s in (1.0, -1.0)]
NON_FINITE = [("off", INF, 0), ("off", -INF, 0), ("off", NAN, 0)]
WILD = WILD_FINITE + NON_FINITE
# the four image corners, both axes on an edge (one corner of the sample inside the image, weight 1/4)
CORNERS = [(("pos", -0.5, 0), ("pos", -0.5, 0)), (("pos", -0.5, 0), ("pos", -0.5, 1)),
           (("pos", -0.5, 1), ("pos", -0.5, 0)), (("pos", -0.5, 1), ("pos", -0.5, 1))]

TILE_H, TILE_W = 8, 32
# LDS windows: (rows above the tile, columns left of it, window rows, window columns).  dcnv2_il / il2 / il16: rows y0-6 .. y0+13,
# columns x0-8 .. x0+39 (ops.dcn_offset_stats); dcnv2_ws: rows y0-5 .. y0+12, columns x0-6 .. x0+37.
WINDOW_IL = (6, 8, 20, 48)
WINDOW_WS = (5, 6, 18, 44)
WINDOWS = {"il": WINDOW_IL, "il2": WINDOW_IL, "il16": WINDOW_IL, "ws": WINDOW_WS}
SEAM_SLOTS = ("before", "first", "last", "after")      # floor(p) at window row / column -1, 0, size - 2, size - 1


def in_window(fy, fx, y0, x0, win=WINDOW_IL):
    """the kernels' window test on floor(p): both corners of either axis inside the window of the tile at (y0, x0)"""
    my, mx, ph, pw = win
    ry, rx = fy - (y0 - my), fx - (x0 - mx)
    return (ry >= 0) & (ry <= ph - 2) & (rx >= 0) & (rx <= pw - 2)


def entry_offset(entry, base, size):
    """the fp32 offset that puts `entry` at a sample whose undisplaced position is `base` on an axis of length `size`"""
    kind, a, b = entry
    return F32(a) if kind == "off" else F32(F32(a + b * size) - F32(base))


# ---- builders ------------------------------------------------------------------------------------------------------------------
def _hash(i, salt):
    return (i.astype(np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) % np.uint64(2 ** 32)


def tier_entries(tier):
    return {"edge": EDGE, "wild": WILD, "ordinary": []}[tier]


def dcn_offsets(tier, n, dg, h, w, seed=0, share=4):
    """(offset (n, 18 dg, h, w) fp32, tag (n, dg, 9, h, w, 2) int): sigma = 1 offsets with, at one sample in `share` chosen by a fixed
    hash, ONE axis (chosen by the hash) replaced by an entry of the tier's table; tag = the entry's index + 1 per axis (0: ordinary).
    tier "edge" also places the four corner entries (both axes), tier "seam" the window seams of both window geometries."""
    rng = np.random.RandomState(1000 + seed)
    off = rng.standard_normal((n, dg, 9, 2, h, w)).astype(F32)
    tag = np.zeros((n, dg, 9, h, w, 2), np.int32)
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if tier == "seam":
        _place_seams(off, tag, h, w)
        return off.reshape(n, dg * 18, h, w), tag
    table = tier_entries(tier)
    T = len(table)
    idx = np.arange(n * dg * 9 * h * w).reshape(n, dg, 9, h, w)
    hs = _hash(idx, seed)
    special = (hs >> np.uint64(7)) % np.uint64(share) == 0
    pick = ((hs >> np.uint64(11)) % np.uint64(2 * T + (len(CORNERS) if tier == "edge" else 0))).astype(np.int64)
    for k in range(9):
        by, bx = (gy - 1 + k // 3).astype(F32), (gx - 1 + k % 3).astype(F32)
        for e in range(T):
            for axis, (base, size) in enumerate(((by, h), (bx, w))):
                m = special[:, :, k] & (pick[:, :, k] == 2 * e + axis)
                val = np.broadcast_to(entry_offset(table[e], base, size), m.shape)
                off[:, :, k, axis][m] = val[m]
                tag[:, :, k, :, :, axis][m] = e + 1
        if tier == "edge":
            for ci, (ey, ex) in enumerate(CORNERS):
                m = special[:, :, k] & (pick[:, :, k] == 2 * T + ci)
                off[:, :, k, 0][m] = np.broadcast_to(entry_offset(ey, by, h), m.shape)[m]
                off[:, :, k, 1][m] = np.broadcast_to(entry_offset(ex, bx, w), m.shape)[m]
                tag[:, :, k, :, :, 0][m] = T + 1 + ci
                tag[:, :, k, :, :, 1][m] = T + 1 + ci
    return off.reshape(n, dg * 18, h, w), tag


def seam_targets(y0, x0, h, w, win):
    """[(axis, slot, floor)]: the window rows / columns -1, 0, size - 2, size - 1 of the tile at (y0, x0), as image coordinates"""
    my, mx, ph, pw = win
    out = []
    for slot, r in zip(SEAM_SLOTS, (-1, 0, ph - 2, ph - 1)):
        out.append((0, slot, y0 - my + r))
    for slot, c in zip(SEAM_SLOTS, (-1, 0, pw - 2, pw - 1)):
        out.append((1, slot, x0 - mx + c))
    return out


def seam_plan(h, w):
    """[(win name, y, x, axis, slot, floor, frac)] -- every seam placement whose two corners on the seam axis lie inside the image (a
    sample over the image edge reads zeros on either path and could not show a seam that is off by one), from the pixels of each
    tile's first and last row and column"""
    plan = []
    for wname, win in (("il", WINDOW_IL), ("ws", WINDOW_WS)):
        for y0 in range(0, h, TILE_H):
            for x0 in range(0, w, TILE_W):
                ys = sorted({y0, min(y0 + TILE_H, h) - 1})
                xs = sorted({x0, min(x0 + TILE_W, w) - 1})
                for axis, slot, fl in seam_targets(y0, x0, h, w, win):
                    if not (0 <= fl <= (h, w)[axis] - 2):
                        continue
                    for y in ys:
                        for x in xs:
                            for frac in (0.0, 0.5):
                                plan.append((wname, y, x, axis, slot, fl, frac))
    return plan


def _place_seams(off, tag, h, w):
    """one seam placement per (pixel, tap, group) slot, round robin over taps and groups; the other axis stays at the pixel's own
    undisplaced coordinate + 0.25 (inside every window)"""
    n, dg = off.shape[:2]
    for i, (wname, y, x, axis, slot, fl, frac) in enumerate(seam_plan(h, w)):
        k, g = i % 9, (i // 9) % dg
        by, bx = F32(y - 1 + k // 3), F32(x - 1 + k % 3)
        tgt = [F32(y + 0.25), F32(x + 0.25)]
        tgt[axis] = F32(fl + frac)
        off[:, g, k, 0, y, x] = tgt[0] - by
        off[:, g, k, 1, y, x] = tgt[1] - bx
        tag[:, g, k, y, x, :] = 0
        tag[:, g, k, y, x, axis] = 1 + SEAM_SLOTS.index(slot) + (4 if wname == "ws" else 0)


def dcn_all_invalid(off, h, w, pixels, seed=0):
    """every tap of every group of the chosen pixels invalid, by the wild table in turn (non-finite entries included) on one axis"""
    n, c18 = off.shape[:2]
    o = off.reshape(n, c18 // 18, 9, 2, h, w).copy()
    invalid = [e for e in WILD if not (e[0] == "pos")] + [("pos", 4.0, 1), ("pos", -4.0, -1), ("pos", -1.0, 0), ("pos", 0.0, 1)]
    i = seed
    for (y, x) in pixels:
        for g in range(o.shape[1]):
            for k in range(9):
                e = invalid[i % len(invalid)]
                axis = (i // len(invalid)) % 2
                base, size = ((y - 1 + k // 3), h) if axis == 0 else ((x - 1 + k % 3), w)
                o[:, g, k, axis, y, x] = entry_offset(e, F32(base), size)
                i += 1
    return o.reshape(n, c18, h, w)


def warp_flow(tier, n, h, w, seed=0, share=4):
    """(flow (n, 2, h, w) fp32, tag (n, h, w, 2)): sigma = 1 flow, one pixel in `share` with one axis at a table entry (flow channel 0
    is x, channel 1 is y); tier "edge" also places the four corners"""
    rng = np.random.RandomState(2000 + seed)
    flow = rng.standard_normal((n, 2, h, w)).astype(F32)
    tag = np.zeros((n, h, w, 2), np.int32)
    table = tier_entries(tier)
    T = len(table)
    if T == 0:
        return flow, tag
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    hs = _hash(np.arange(n * h * w).reshape(n, h, w), seed)
    special = (hs >> np.uint64(7)) % np.uint64(share) == 0
    pick = ((hs >> np.uint64(11)) % np.uint64(2 * T + (len(CORNERS) if tier == "edge" else 0))).astype(np.int64)
    for e in range(T):
        for axis, (base, size, ch) in enumerate(((gy.astype(F32), h, 1), (gx.astype(F32), w, 0))):
            m = special & (pick == 2 * e + axis)
            flow[:, ch][m] = np.broadcast_to(entry_offset(table[e], base, size), m.shape)[m]
            tag[..., axis][m] = e + 1
    if tier == "edge":
        for ci, (ey, ex) in enumerate(CORNERS):
            m = special & (pick == 2 * T + ci)
            flow[:, 1][m] = np.broadcast_to(entry_offset(ey, gy.astype(F32), h), m.shape)[m]
            flow[:, 0][m] = np.broadcast_to(entry_offset(ex, gx.astype(F32), w), m.shape)[m]
            tag[m] = T + 1 + ci
    return flow, tag


def warp_all_invalid(flow, pixels):
    """the chosen pixels sample outside the image (zeros padding: +0.0), by the wild table in turn"""
    f = flow.copy()
    n, _, h, w = f.shape
    for i, (y, x) in enumerate(pixels):
        e = WILD[i % len(WILD)]
        axis = (i // len(WILD)) % 2
        f[:, 1 - axis, y, x] = entry_offset(e, F32((y, x)[axis]), (h, w)[axis])
    return f


# ---- positions -----------------------------------------------------------------------------------------------------------------
def dcn_positions(offset, dg):
    """(py, px) fp32 (n, dg, 9, h, w): fl(fl(pixel + (tap - 1)) + offset)"""
    n, _, h, w = offset.shape
    o = offset.reshape(n, dg, 9, 2, h, w).astype(F32)
    gy, gx = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    ky = (np.arange(9) // 3 - 1).astype(F32).reshape(1, 1, 9, 1, 1)
    kx = (np.arange(9) % 3 - 1).astype(F32).reshape(1, 1, 9, 1, 1)
    with np.errstate(all="ignore"):
        return ((gy + ky).astype(F32) + o[:, :, :, 0]).astype(F32), ((gx + kx).astype(F32) + o[:, :, :, 1]).astype(F32)


def heads_offsets(heads, D):
    """AdaptBlockOffset's tail in fp32 as the kernels evaluate it: offset = fl(fl(fl(T0 ry + T1 rx) - ry) + t) (ry, rx in {-1, 0, 1}:
    the products are exact, fused or not), mask = sigmoid -> (offset (n, 18 D, h, w) fp32, mask (n, 9 D, h, w) float64)"""
    n, _, h, w = heads.shape
    T = heads[:, :4 * D].reshape(n, D, 4, 1, h, w).astype(F32)
    t = heads[:, 4 * D:6 * D].reshape(n, D, 2, 1, h, w).astype(F32)
    ry = (np.arange(9) // 3 - 1).astype(F32).reshape(1, 1, 9, 1, 1)
    rx = (np.arange(9) % 3 - 1).astype(F32).reshape(1, 1, 9, 1, 1)
    with np.errstate(all="ignore"):
        dy = (((T[:, :, 0] * ry).astype(F32) + (T[:, :, 1] * rx).astype(F32)).astype(F32) - ry).astype(F32) + t[:, :, 0]
        dx = (((T[:, :, 2] * ry).astype(F32) + (T[:, :, 3] * rx).astype(F32)).astype(F32) - rx).astype(F32) + t[:, :, 1]
        m = 1.0 / (1.0 + np.exp(-heads[:, 6 * D:].astype(np.float64)))
    off = np.stack([dy.astype(F32), dx.astype(F32)], 3).reshape(n, D * 18, h, w)
    return off, m


def heads_from_offsets(off, tag, D, seed=0):
    """(n, 15 D, h, w) heads with T = identity, so that (T . R) - R + t = t exactly at every tap: per (pixel, group) the translation
    is the offset `off` holds at ONE tap -- the tap that carries a table entry (tag != 0) if there is one, else a hashed one -- and that
    tap's position is the table's, reached through the heads-mode formula; the other eight taps move with it.  Mask logits N(0, 2)."""
    n, _, h, w = off.shape
    o = off.reshape(n, D, 9, 2, h, w)
    has = (tag != 0).any(-1)                                                    # (n, D, 9, h, w)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    fallback = (yy * w + xx + np.arange(D).reshape(D, 1, 1)) % 9                  # (D, h, w)
    k = np.where(has.any(2), has.argmax(2), fallback[None])                      # (n, D, h, w)
    t = np.take_along_axis(o, k[:, :, None, None], axis=2)[:, :, 0]              # (n, D, 2, h, w)
    heads = np.zeros((n, 15 * D, h, w), F32)
    heads[:, 0:4 * D:4] = 1.0
    heads[:, 3:4 * D:4] = 1.0
    heads[:, 4 * D:6 * D] = t.reshape(n, 2 * D, h, w)
    heads[:, 6 * D:] = np.random.RandomState(3000 + seed).standard_normal((n, 9 * D, h, w)).astype(F32) * 2
    return heads, k


def warp_positions(flow, flow2=None, align=True):
    """(iy, ix) fp32 (n, h, w) of flow_warp: the reference's normalise / un-normalise pair, operation by operation"""
    n, _, h, w = flow.shape
    f = flow.astype(F32)
    with np.errstate(all="ignore"):
        if flow2 is not None:
            f = (f + flow2.astype(F32)).astype(F32)
        gy, gx = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
        out = []
        for g, d, size in ((gy + f[:, 1], 1, h), (gx + f[:, 0], 0, w)):
            g = g.astype(F32)
            nn = ((F32(2.0) * g).astype(F32) / F32(max(size - 1, 1))).astype(F32) - F32(1.0)
            nn = nn.astype(F32)
            if align:
                p = (((nn + F32(1.0)).astype(F32) / F32(2.0)).astype(F32) * F32(size - 1)).astype(F32)
            else:
                p = ((((nn + F32(1.0)).astype(F32) * F32(size)).astype(F32) - F32(1.0)).astype(F32) / F32(2.0)).astype(F32)
            out.append(p)
    return out[0], out[1]


def pwc_positions(flow, h, w, fs=1, fmul=1.0):
    """[(iy, ix)] x 2 fp32 (n, h, w): pwc_backwarp's position with ((g + 1) size - 1) rounded in two steps, and fused"""
    n = flow.shape[0]
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    f = flow.astype(F32)[:, :, yy // fs, xx // fs]
    res = [[], []]
    with np.errstate(all="ignore"):
        for ch, coord, size in ((1, yy, h), (0, xx, w)):
            fv = (f[:, ch] * F32(fmul)).astype(F32)
            base = (F32(-1.0) + ((2 * coord + 1).astype(F32) / F32(size)).astype(F32)).astype(F32)
            g = (base + (fv / ((F32(size) - F32(1.0)) / F32(2.0)).astype(F32)).astype(F32)).astype(F32)
            g1 = (g + F32(1.0)).astype(F32)
            two = (((g1 * F32(size)).astype(F32) - F32(1.0)).astype(F32) / F32(2.0)).astype(F32)
            fused = ((g1.astype(np.float64) * size - 1.0).astype(F32) / F32(2.0)).astype(F32)      # one rounding of g1 * size - 1
            res[0].append(two)
            res[1].append(fused)
    return [tuple(res[0]), tuple(res[1])]


# ---- float64 interpolation -----------------------------------------------------------------------------------------------------
def _corners(py, px, h, w, valid):
    """per sample: four (iy, ix, weight float64, inside bool), weights from the fp32 position in float64; `valid` gates all four"""
    ok = valid & np.isfinite(py) & np.isfinite(px)
    p64y, p64x = np.where(ok, py, 0).astype(np.float64), np.where(ok, px, 0).astype(np.float64)
    fy, fx = np.floor(p64y), np.floor(p64x)
    ly, lx = p64y - fy, p64x - fx
    out = []
    for dy, wy in ((0, 1 - ly), (1, ly)):
        for dx, wx in ((0, 1 - lx), (1, lx)):
            cy, cx = fy + dy, fx + dx
            ins = ok & (cy >= 0) & (cy <= h - 1) & (cx >= 0) & (cx <= w - 1)
            out.append((np.clip(cy, 0, h - 1).astype(np.int64), np.clip(cx, 0, w - 1).astype(np.int64), np.where(ins, wy * wx, 0.0), ins,
                        (dy, dx, wy, wx)))
    return out


def dcn_gate(py, px, h, w, variant=None):
    with np.errstate(invalid="ignore"):
        lo = (lambda p: p >= -1) if variant == "gate_ge" else (lambda p: p > -1)
        hi = (lambda p, s: p <= s) if variant == "gate_le" else (lambda p, s: p < s)
        return lo(py) & lo(px) & hi(py, h) & hi(px, w)


def dcn_columns(x, offset, mask, dg, variant=None, tile_window=None):
    """columns (n, c, 9, h, w) float64 = bilinear(x, p) * mask by the contract -- or, with `variant`, by a DELIBERATELY WRONG rule the
    comparisons must catch: "gate_ge" / "gate_le" (the gate -1 <= p, p <= size), "nan0" (a NaN position converted to index 0 and
    taken as valid: NaN weights), "wrap" (a wrapping float-to-int conversion and no float gate), "seam" (fast / slow seam one row and
    column late: the sample at window row / column size - 1 is served from the window and loses its far corners)"""
    n, c, h, w = x.shape
    cpg = c // dg
    py, px = dcn_positions(offset, dg)
    m = np.asarray(mask, np.float64).reshape(n, dg, 9, h, w)
    xg = np.asarray(x, np.float64).reshape(n, dg, cpg, h, w)
    gate = dcn_gate(py, px, h, w, variant)
    if variant == "wrap":
        with np.errstate(all="ignore"):
            wr = lambda p: (np.where(np.isfinite(p), np.floor(p.astype(np.float64)), 0).astype(np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31
            iy, ix = wr(py), wr(px)
            py = np.where(np.isfinite(py) & (np.abs(py) >= 2.0 ** 24), iy, py).astype(F32)
            px = np.where(np.isfinite(px) & (np.abs(px) >= 2.0 ** 24), ix, px).astype(F32)
        gate = np.isfinite(py) & np.isfinite(px)
    val = np.zeros((n, dg, cpg, 9, h, w))
    nidx = np.arange(n).reshape(n, 1, 1, 1, 1)
    gidx = np.arange(dg).reshape(1, dg, 1, 1, 1)
    lose_far = None
    if variant == "seam":
        win = tile_window or WINDOW_IL
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        y0, x0 = yy // TILE_H * TILE_H, xx // TILE_W * TILE_W
        with np.errstate(invalid="ignore"):
            fy, fx = np.floor(py), np.floor(px)
        lose_far = ((fy - (y0 - win[0]) == win[2] - 1), (fx - (x0 - win[1]) == win[3] - 1))
    for cy, cx, wgt, ins, (dy, dx, _, _) in _corners(py, px, h, w, gate):
        if lose_far is not None:
            wgt = np.where((lose_far[0] & (dy == 1)) | (lose_far[1] & (dx == 1)), 0.0, wgt)
        for cc in range(cpg):
            val[:, :, cc] += wgt * xg[nidx, gidx, cc, cy, cx]
    if variant == "nan0":
        with np.errstate(invalid="ignore"):
            val = np.where((np.isnan(py) | np.isnan(px))[:, :, None], NAN, val)
    return (val * m[:, :, None]).reshape(n, c, 9, h, w)


def dcnv2(x, offset, mask, weight, bias, dg, variant=None, tile_window=None):
    """DCNv2 3x3, stride 1, pad 1, float64"""
    col = dcn_columns(x, offset, mask, dg, variant, tile_window)
    n, c, _, h, w = col.shape
    wt = np.asarray(weight, np.float64).reshape(weight.shape[0], c * 9)
    out = np.einsum("ok,nkp->nop", wt, col.reshape(n, c * 9, h * w)).reshape(n, -1, h, w)
    return out if bias is None else out + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)


def dcnv2_backward(x, offset, mask, weight, dy, dg, variant=None, dcol=None):
    """(dx, doffset, dmask, frac_ok) float64 for the cotangent dy (or the column gradient `dcol` (n, c * 9, h, w) itself);
    frac_ok (n, 18 dg, h, w): the position of that offset entry is finite and NOT an integer (d/doffset is one-sided at integers) --
    or the sample is gate-invalid, where doffset is exactly 0 and is compared as such"""
    n, c, h, w = x.shape
    cpg = c // dg
    py, px = dcn_positions(offset, dg)
    gate = dcn_gate(py, px, h, w, variant) & np.isfinite(py) & np.isfinite(px)
    m = np.asarray(mask, np.float64).reshape(n, dg, 9, h, w)
    xg = np.asarray(x, np.float64).reshape(n, dg, cpg, h, w)
    if dcol is None:
        wt = np.asarray(weight, np.float64).reshape(weight.shape[0], c * 9)
        dcol = np.einsum("ok,nop->nkp", wt, np.asarray(dy, np.float64).reshape(n, -1, h * w))
    dcol = np.asarray(dcol, np.float64).reshape(n, dg, cpg, 9, h, w)
    nidx = np.arange(n).reshape(n, 1, 1, 1, 1)
    gidx = np.arange(dg).reshape(1, dg, 1, 1, 1)
    dx = np.zeros((n, dg, cpg, h, w))
    dmask = np.zeros((n, dg, 9, h, w))
    dpy, dpx = np.zeros((n, dg, 9, h, w)), np.zeros((n, dg, 9, h, w))
    for cy, cx, wgt, ins, (sy, sx, wy, wx) in _corners(py, px, h, w, gate):
        for cc in range(cpg):
            v = np.where(ins, xg[nidx, gidx, cc, cy, cx], 0.0)
            d = dcol[:, :, cc]
            dmask += d * wgt * v
            dpy += d * m * v * (1 if sy else -1) * wx
            dpx += d * m * v * (1 if sx else -1) * wy
            np.add.at(dx[:, :, cc], (np.broadcast_to(nidx, cy.shape), np.broadcast_to(gidx, cy.shape), cy, cx), d * m * wgt)
    doff = np.stack([np.where(gate, dpy, 0.0), np.where(gate, dpx, 0.0)], 3).reshape(n, dg * 18, h, w)
    with np.errstate(invalid="ignore"):
        nonint = gate & (py != np.floor(py)) & (px != np.floor(px))
    ok = nonint | ~gate
    frac_ok = np.stack([ok, ok], 3).reshape(n, dg * 18, h, w)
    return dx.reshape(n, c, h, w), doff, dmask.reshape(n, dg * 9, h, w), frac_ok


# ---- flow_warp -----------------------------------------------------------------------------------------------------------------
def _reflect(p, lo2, hi2):
    """aten's reflect_coordinates in fp32, as csrc/flow_warp.hip restates it"""
    if lo2 == hi2:
        return np.zeros_like(p)
    mn, span = F32(lo2) / F32(2), F32(hi2 - lo2) / F32(2)
    with np.errstate(all="ignore"):
        a = np.abs((p - mn).astype(F32))
        extra = np.fmod(a, span).astype(F32)
        flips = np.floor((a / span).astype(F32))
        return np.where(np.fmod(flips, 2) == 0, (extra + mn).astype(F32), ((span - extra).astype(F32) + mn).astype(F32)).astype(F32)


def flow_warp(x, flow, padding_mode="zeros", flow2=None, interpolation="bilinear", align=True):
    """(out float64, pinned bool (n, h, w)): `pinned` is False exactly where the contract leaves the value open -- a non-finite
    position under border / reflection, reflection at |position| >= 2^24"""
    n, c, h, w = x.shape
    iy, ix = warp_positions(flow, flow2, align)
    finite = np.isfinite(iy) & np.isfinite(ix)
    pinned = np.ones((n, h, w), bool)
    with np.errstate(invalid="ignore"):
        if padding_mode == "reflection":
            pinned = finite & (np.abs(iy) < 2.0 ** 24) & (np.abs(ix) < 2.0 ** 24)
            iy = _reflect(iy, 0, 2 * (h - 1)) if align else _reflect(iy, -1, 2 * h - 1)
            ix = _reflect(ix, 0, 2 * (w - 1)) if align else _reflect(ix, -1, 2 * w - 1)
        if padding_mode != "zeros":
            pinned = pinned & finite
            iy, ix = np.clip(iy, F32(0), F32(h - 1)), np.clip(ix, F32(0), F32(w - 1))
    x64 = np.asarray(x, np.float64)
    nidx = np.arange(n).reshape(n, 1, 1)
    out = np.zeros((n, c, h, w))
    if interpolation == "nearest":
        ok = np.isfinite(iy) & np.isfinite(ix)
        ry, rx = np.rint(np.where(ok, iy, -9)), np.rint(np.where(ok, ix, -9))      # round half to even, as aten
        ins = ok & (ry >= 0) & (ry <= h - 1) & (rx >= 0) & (rx <= w - 1)
        cy, cx = np.clip(ry, 0, h - 1).astype(np.int64), np.clip(rx, 0, w - 1).astype(np.int64)
        for cc in range(c):
            out[:, cc] = np.where(ins, x64[nidx, cc, cy, cx], 0.0)
        return out, pinned
    for cy, cx, wgt, ins, _ in _corners(iy, ix, h, w, np.ones((n, h, w), bool)):
        for cc in range(c):
            out[:, cc] += wgt * x64[nidx, cc, cy, cx]
    return out, pinned


def flow_warp_backward(x, flow, dout, flow2=None):
    """(dx, dflow, frac_ok (n, 2, h, w)) float64, zeros padding; d(position) / d(flow) = 1"""
    n, c, h, w = x.shape
    iy, ix = warp_positions(flow, flow2)
    x64, g = np.asarray(x, np.float64), np.asarray(dout, np.float64)
    nidx = np.arange(n).reshape(n, 1, 1)
    dx = np.zeros((n, c, h, w))
    dfy, dfx = np.zeros((n, h, w)), np.zeros((n, h, w))
    anyin = np.zeros((n, h, w), bool)
    for cy, cx, wgt, ins, (sy, sx, wy, wx) in _corners(iy, ix, h, w, np.ones((n, h, w), bool)):
        anyin |= ins
        for cc in range(c):
            v = np.where(ins, x64[nidx, cc, cy, cx], 0.0)
            dfy += g[:, cc] * v * (1 if sy else -1) * wx
            dfx += g[:, cc] * v * (1 if sx else -1) * wy
            np.add.at(dx[:, cc], (np.broadcast_to(nidx, cy.shape), cy, cx), g[:, cc] * wgt)
    with np.errstate(invalid="ignore"):
        nonint = np.isfinite(iy) & np.isfinite(ix) & (iy != np.floor(iy)) & (ix != np.floor(ix))
    ok = nonint | ~anyin
    return dx, np.stack([dfx, dfy], 1), np.stack([ok, ok], 1), anyin


# ---- pwc_backwarp --------------------------------------------------------------------------------------------------------------
def pwc_backwarp(x, flow, fs=1, fmul=1.0):
    """[(out float64, mask float64 (n, 1, h, w), ones)] for the two roundings of the position; out = warped x mask, mask = (sum of the
    in-image corner weights > 0.999), 0 at a non-finite position"""
    n, c, h, w = x.shape
    x64 = np.asarray(x, np.float64)
    nidx = np.arange(n).reshape(n, 1, 1)
    res = []
    for iy, ix in pwc_positions(flow, h, w, fs, fmul):
        out, ones = np.zeros((n, c, h, w)), np.zeros((n, h, w))
        for cy, cx, wgt, ins, _ in _corners(iy, ix, h, w, np.ones((n, h, w), bool)):
            ones += wgt
            for cc in range(c):
                out[:, cc] += wgt * x64[nidx, cc, cy, cx]
        mask = (ones > 0.999).astype(np.float64)
        res.append((out * mask[:, None], mask[:, None], ones))
    return res


def pwc_flow(tier, n, h, w, fs=1, seed=0):
    """flow (n, 2, h / fs, w / fs) for pwc_backwarp (position = pixel + flow size / (size - 1)): sigma = 1, a quarter of the pixels at
    table entries, and -- tier "edge" -- pixels whose summed corner weights sit 2^-13 on either side of 0.999"""
    fh, fw = h // fs, w // fs
    flow, tag = warp_flow(tier, n, fh, fw, seed)
    # entry_offset gives position - pixel in flow-grid units; the kernel scales by size / (size - 1) at the full size
    flow[:, 0] *= F32((w - 1) / w * fs)
    flow[:, 1] *= F32((h - 1) / h * fs)
    if tier == "edge" and fs == 1:
        k = 0
        for y in range(1, h - 1):
            for x in range(1, w - 1):
                if tag[:, y, x].any() or (y * w + x) % 7:
                    continue
                d = 0.001 + (2.0 ** -13) * (1 if k % 2 else -1)        # the lost weight: ones = 1 - d
                if k % 4 < 2:
                    flow[:, 0, y, x] = F32((-d - x) * (w - 1) / w)      # position -d on x: ones = 1 - d
                    flow[:, 1, y, x] = F32(0.0)
                else:
                    flow[:, 1, y, x] = F32((h - 1 + d - y) * (h - 1) / h)
                    flow[:, 0, y, x] = F32(0.0)
                k += 1
    return flow
