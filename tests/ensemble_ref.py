"""Self-ensemble inference restated with numpy, nothing of eavsr_amd imported: the eight modes (`g`, `inv`), where the
frame's samples lie after padding and transforming (`valid_region`), the blend with its three separately rounded float32 steps
(`blend_oracle`, `ensemble_blend`), and the address arithmetic of csrc/blend.hip's four kernels, workgroup by workgroup and lane by
lane (`dihedral_transcription`, `blend_dihedral_transcription`): every load asserts that it lies inside its source and that a wide
load is aligned, every store that it lies inside its destination and is aligned; the dihedral stores each sample exactly once."""
import numpy as np

from tests.tile_ref import Memory, row_blocks
from tests.tile_ref import blend_oracle as tile_blend_oracle

F32 = np.float32
LANES, ROWS, TILE, PITCH = 64, 4, 64, 65


# ------------------------------------------------------------------------------------------------------------- the definitions
def g(x, k):
    a = x[..., ::-1] if k & 1 else x
    b = a[..., ::-1, :] if k & 2 else a
    return b.swapaxes(-1, -2) if k & 4 else b


def inv(z, k):
    u = z.swapaxes(-1, -2) if k & 4 else z
    a = u[..., ::-1] if k & 1 else u
    return a[..., ::-1, :] if k & 2 else a


def valid_region(k, h, w, H, W, s):
    """(r0, r1, c0, c1) inside the SR frame of mode k: the issue's table, SH = s H, SW = s W"""
    SH, SW = s * H, s * W
    by_h = (SH - s * h, SH) if k & 2 else (0, s * h)      # along the frame's own rows
    by_w = (SW - s * w, SW) if k & 1 else (0, s * w)
    return (by_w + by_h) if k & 4 else (by_h + by_w)


def weight(modes):
    return F32(1) / F32(len(modes))


def blend_oracle(acc, sr, k, Y0, X0, wy, wx):
    """acc[..., Y0 + y, X0 + x] = acc + ((wy[y] * wx[x]) * inv_k(sr)[..., y, x]), in place: tile_ref's statement on inv_k(sr)"""
    return tile_blend_oracle(acc, np.ascontiguousarray(inv(sr, k)), Y0, X0, wy, wx)


def ensemble_blend(per_tile_mode, tiles, modes, h, w, s, wy_rows, wx_rows, ncols):
    """`forward_ensemble`'s contract: per_tile_mode[ti][mi] is the SR clip (n, F, C, ., .) of tile ti under modes[mi], cut to its valid
    region, still in the transformed orientation; wy_rows / wx_rows: float32 (rows of tiles, s th) / (columns of tiles, s tw)"""
    first = np.asarray(per_tile_mode[0][0])
    acc = np.zeros(first.shape[:3] + (s * h, s * w), F32)
    wgt = weight(modes)
    for ti, (y0, _, x0, _) in enumerate(tiles):
        wy = (wy_rows[ti // ncols] * wgt).astype(F32)      # fp32(wy * weight), once
        for mi, k in enumerate(modes):
            blend_oracle(acc, np.ascontiguousarray(per_tile_mode[ti][mi], dtype=F32), k, s * y0, s * x0, wy, wx_rows[ti % ncols])
    return acc


# ------------------------------------------------------------------------------------------------------------- the kernels, restated
def _align_of(addr):
    return 16 if addr % 16 == 0 else (8 if addr % 8 == 0 else 4)


def _load_quad(mem, addr, align, widths):
    widths[align] += 16 // align
    return b"".join(mem.load(addr + j, align, align) for j in range(0, 16, align))


def _store_quad(mem, addr, align, data, widths):
    widths[align] += 16 // align
    for j in range(0, 16, align):
        mem.store(addr + j, data[j:j + align], align)


def _reversed_words(q):
    return b"".join(q[4 * j:4 * j + 4] for j in (3, 2, 1, 0))


def dihedral_transcription(x, k, bases=(0, 0), grid_x=None):
    """csrc/blend.hip's two dihedral kernels on x float32 (F, C, H, W); `bases`: the byte addresses of in and out (multiples of 4)
    -> (g_k(x) as the kernel writes it, {access width: count})"""
    x = np.ascontiguousarray(x, dtype=F32)
    F, C, H, W = x.shape
    src, dst = Memory(x, bases[0], 4), Memory(np.zeros(x.size, F32), bases[1], 4)
    stored = np.zeros(x.size, np.int32)
    widths = {16: 0, 8: 0, 4: 0}
    hflip, vflip = k & 1, (k >> 1) & 1

    def put(addr, data, align):
        at = (addr - bases[1]) // 4
        stored[at:at + len(data) // 4] += 1
        if len(data) == 16:
            _store_quad(dst, addr, align, data, widths)
        else:
            widths[4] += 1
            dst.store(addr, data, 4)

    for f in range(F):
        for c in range(C):
            plane = f * C + c
            s0, d0 = bases[0] + 4 * plane * H * W, bases[1] + 4 * plane * H * W
            if k & 4:
                ntx, nty = -(-W // TILE), -(-H // TILE)
                for b in range(ntx * nty):
                    ty, tx = b // ntx, b % ntx
                    r0, q0 = ty * TILE, tx * TILE
                    rows, cols = min(TILE, H - r0), min(TILE, W - q0)
                    lds = {}
                    for tyi in range(ROWS):
                        for l in range(LANES):
                            if l < cols:
                                for rr in range(tyi, rows, ROWS):
                                    widths[4] += 1
                                    lds[rr * PITCH + l] = src.load(s0 + 4 * ((r0 + rr) * W + q0 + l), 4, 4)
                    for tyi in range(ROWS):
                        for cc in range(tyi, cols, ROWS):
                            banks = set()
                            for l in range(LANES):
                                if l < rows:
                                    banks.add((l * PITCH + cc) % 64)
                                    j = H - 1 - (r0 + l) if vflip else r0 + l
                                    i = W - 1 - (q0 + cc) if hflip else q0 + cc
                                    put(d0 + 4 * (i * H + j), lds[l * PITCH + cc], 4)
                            assert len(banks) == rows, "a column read of the tile touches every LDS bank at most once"
            else:
                gx = row_blocks(H, F * C) if grid_x is None else grid_x
                quads = W // 4
                for bx in range(gx):
                    for tyi in range(ROWS):
                        for y in range(bx * ROWS + tyi, H, gx * ROWS):
                            srow = s0 + 4 * ((H - 1 - y if vflip else y) * W)
                            drow = d0 + 4 * y * W
                            d_al = _align_of(drow)
                            tail = srow + 4 * (W & 3)
                            s_al = _align_of(tail if hflip else srow)
                            for xv in range(quads):
                                if hflip:
                                    q = _reversed_words(_load_quad(src, tail + 16 * (quads - 1 - xv), s_al, widths))
                                else:
                                    q = _load_quad(src, srow + 16 * xv, s_al, widths)
                                put(drow + 16 * xv, q, d_al)
                            for xt in range(4 * quads, W):
                                widths[4] += 1
                                put(drow + 4 * xt, src.load(srow + 4 * (W - 1 - xt if hflip else xt), 4, 4), 4)
    assert (stored == 1).all(), "every output sample is stored exactly once"
    return dst.array(F32, (F, C, W, H) if k & 4 else (F, C, H, W)), widths


def blend_dihedral_transcription(acc, sr_store, sr_offset, sr_shape, sr_strides, k, Y0, X0, wy, wx, bases=(0, 0, 0, 0), grid_x=None):
    """csrc/blend.hip's two blend kernels (k in 0 .. 7; 0 is the tile blend): acc float32 (n, F, C, SH, SW) contiguous; the source is the
    strided view of the flat float32 array `sr_store` that starts `sr_offset` elements in, with `sr_shape` (n, F, C, rows, row) --
    (tw, th) for a transposed mode -- and element strides `sr_strides` (n, f, c, rows; unit along a row); wy (th,), wx (tw,).
    `bases`: the byte addresses of acc, sr_store, wy, wx (multiples of 4).  -> (the new acc, {access width: how many accesses the
    QUADS of the rows kernel made at it}; the single words of a row's tail, of wy and of the transposing kernel are not counted)"""
    n, F, C, SH, SW = acc.shape
    rows_s, row_s = sr_shape[3:]
    th, tw = (row_s, rows_s) if k & 4 else (rows_s, row_s)
    assert 0 <= k <= 7 and tuple(sr_shape[:3]) == (n, F, C) and 0 <= Y0 and 0 <= X0 and Y0 + th <= SH and X0 + tw <= SW
    assert wy.shape == (th,) and wx.shape == (tw,)
    sn, sf, sc, sy = sr_strides
    assert all(b % 4 == 0 for b in bases) and min(sn, sf, sc) >= 0 and sy >= row_s
    A, S, WY, WX = (Memory(a, b, 4) for a, b in zip((acc, sr_store, wy, wx), bases))
    widths = {16: 0, 8: 0, 4: 0}
    hflip, vflip = k & 1, (k >> 1) & 1
    f32 = lambda raw: np.frombuffer(raw, F32)

    def blend(a, wyv, wxv, v):
        return F32(a + F32(F32(wyv * wxv) * v))

    def word(mem, addr):
        return f32(mem.load(addr, 4, 4))[0]

    for bz in range(n * F):
        nn, f = bz // F, bz % F
        for by in range(C):
            plane = bz * C + by
            dst = bases[0] + 4 * ((plane * SH + Y0) * SW + X0)
            src = bases[1] + 4 * (sr_offset + nn * sn + f * sf + by * sc)
            if k & 4:
                ntx, nty = -(-th // TILE), -(-tw // TILE)      # source columns run over th, source rows over tw
                for b in range(ntx * nty):
                    ty, tx = b // ntx, b % ntx
                    r0, q0 = ty * TILE, tx * TILE
                    rows, cols = min(TILE, tw - r0), min(TILE, th - q0)
                    lds = {}
                    for tyi in range(ROWS):
                        for l in range(LANES):
                            if l < cols:
                                for rr in range(tyi, rows, ROWS):
                                    lds[rr * PITCH + l] = word(S, src + 4 * ((r0 + rr) * sy + q0 + l))
                    for tyi in range(ROWS):
                        for l in range(LANES):
                            if l < rows:
                                x = tw - 1 - (r0 + l) if hflip else r0 + l
                                wxv = word(WX, bases[3] + 4 * x)
                                for cc in range(tyi, cols, ROWS):
                                    y = th - 1 - (q0 + cc) if vflip else q0 + cc
                                    at = dst + 4 * (y * SW + x)
                                    res = blend(word(A, at), word(WY, bases[2] + 4 * y), wxv, lds[l * PITCH + cc])
                                    A.store(at, res.tobytes(), 4)
            else:
                gx = row_blocks(th, n * F * C) if grid_x is None else grid_x
                quads = tw // 4
                w_al = _align_of(bases[3])
                for bx in range(gx):
                    for tyi in range(ROWS):
                        for y in range(bx * ROWS + tyi, th, gx * ROWS):
                            arow = dst + 4 * y * SW
                            srow = src + 4 * (th - 1 - y if vflip else y) * sy
                            tail = srow + 4 * (tw & 3)
                            wyv = word(WY, bases[2] + 4 * y)
                            a_al, s_al = _align_of(arow), _align_of(tail if hflip else srow)
                            for xv in range(quads):
                                a = f32(_load_quad(A, arow + 16 * xv, a_al, widths))
                                w = f32(_load_quad(WX, bases[3] + 16 * xv, w_al, widths))
                                if hflip:
                                    v = f32(_reversed_words(_load_quad(S, tail + 16 * (quads - 1 - xv), s_al, widths)))
                                else:
                                    v = f32(_load_quad(S, srow + 16 * xv, s_al, widths))
                                res = np.array([blend(a[j], wyv, w[j], v[j]) for j in range(4)], F32).tobytes()
                                _store_quad(A, arow + 16 * xv, a_al, res, widths)
                            for x in range(4 * quads, tw):
                                v = word(S, srow + 4 * (tw - 1 - x if hflip else x))
                                res = blend(word(A, arow + 4 * x), wyv, word(WX, bases[3] + 4 * x), v)
                                A.store(arow + 4 * x, res.tobytes(), 4)
    return A.array(F32, acc.shape), widths
