"""Spatial tiling restated with scalar numpy, nothing of eavsr_amd imported: the plan (`plan_axis`, `plan_tiles`), the
blending weights (`weights`), the window ingest (`window_oracle`: slice, np.pad, `np.float32(v) / 255`), the blend (`blend_oracle`:
numpy float32 products and sums, each rounded on its own -- numpy fuses nothing), the blend of whole tiles (`blend_tiles`), and the
two kernels' own address arithmetic, workgroup by workgroup and lane by lane (`ingest_window_transcription`,
`tile_blend_transcription`): every load asserts that it lies inside its source and that a wide load is aligned, every store that it
lies inside the output, is aligned, and -- for the ingest -- is the only store to its samples."""
import numpy as np

F32 = np.float32
LANES, ROWS = 64, 4
U8_PLANES, U8_INTERLEAVED, F32_PLANES = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------- plan and weights
def plan_axis(size, tile, overlap):
    if size <= tile:
        return [(0, size)]
    out, a = [], 0
    while a + tile < size:
        out.append((a, a + tile))
        a += tile - overlap
    out.append((size - tile, size))
    return out


def plan_tiles(h, w, tile, overlap):
    th, tw = (tile, tile) if isinstance(tile, int) else tile
    return [(y0, y1, x0, x1) for y0, y1 in plan_axis(h, th, overlap) for x0, x1 in plan_axis(w, tw, overlap)]


def raw_weight(X, a, b, size, s):
    dl = X - s * a + 0.5 if a > 0 else np.inf
    dr = s * b - X - 0.5 if b < size else np.inf
    m = min(dl, dr)
    return 1.0 if np.isinf(m) else m


def weights(size, windows, s):
    """float32 (k, s * tile_len), sample by sample in float64, rounded once"""
    out = np.zeros((len(windows), s * (windows[0][1] - windows[0][0])), F32)
    for k, (a, b) in enumerate(windows):
        for X in range(s * a, s * b):
            total = np.float64(0)
            for c, d in windows:
                if s * c <= X < s * d:
                    total += np.float64(raw_weight(X, c, d, size, s))
            out[k, X - s * a] = F32(np.float64(raw_weight(X, a, b, size, s)) / total)
    return out


def coverage(size, windows, s):
    """how many windows cover each SR sample"""
    cover = np.zeros(s * size, np.int64)
    for a, b in windows:
        cover[s * a:s * b] += 1
    return cover


# ------------------------------------------------------------------------------------------------------------- the two definitions
def window_oracle(x, y0, x0, wh, ww, H, W, mode, hwc=False):
    """x uint8 / float32 (F, C, h, w), or uint8 (F, h, w, 3) with hwc -> float32 (F, C, H, W)"""
    x = np.asarray(x)
    if hwc:
        x = x.transpose(0, 3, 1, 2)
    part = np.ascontiguousarray(x[:, :, y0:y0 + wh, x0:x0 + ww])
    padded = np.pad(part, ((0, 0), (0, 0), (0, H - wh), (0, W - ww)), mode=mode)
    if x.dtype == np.uint8:
        return padded.astype(F32) / F32(255)
    return padded


def blend_oracle(acc, sr, Y0, X0, wy, wx):
    """acc (n, F, C, SH, SW) float32, in place: acc[..., Y0 + y, X0 + x] += (wy[y] * wx[x]) * sr[..., y, x]"""
    assert acc.dtype == F32 and sr.dtype == F32 and wy.dtype == F32 and wx.dtype == F32
    th, tw = sr.shape[-2:]
    w2 = wy[:, None] * wx[None, :]            # float32 * float32 -> float32, rounded
    prod = w2 * sr                            # rounded
    acc[..., Y0:Y0 + th, X0:X0 + tw] = acc[..., Y0:Y0 + th, X0:X0 + tw] + prod      # rounded
    return acc


def blend_tiles(tiles_sr, tiles, h, w, s, tile, overlap):
    """the frame from per-tile SR tensors (n, F, C, s th, s tw) in plan order -- `forward_tiled`'s contract"""
    th, tw = (tile, tile) if isinstance(tile, int) else tile
    rows, cols = plan_axis(h, th, overlap), plan_axis(w, tw, overlap)
    wy, wx = weights(h, rows, s), weights(w, cols, s)
    assert tiles == plan_tiles(h, w, tile, overlap)
    first = np.asarray(tiles_sr[0])
    acc = np.zeros(first.shape[:3] + (s * h, s * w), F32)
    for ti, ((y0, _, x0, _), sr) in enumerate(zip(tiles, tiles_sr)):
        blend_oracle(acc, np.ascontiguousarray(sr, dtype=F32), s * y0, s * x0, wy[ti // len(cols)], wx[ti % len(cols)])
    return acc


# ------------------------------------------------------------------------------------------------------------- the kernels, restated
def src_index(i, s, edge):
    assert 0 <= i < 2 ** 32 and 1 <= s < 2 ** 31
    if i < s:
        return i
    if edge or s == 1:
        return s - 1
    period = 2 * (s - 1)
    m = i % period
    return m if m < s else period - m


def row_blocks(H, planes):
    want = (H + ROWS - 1) // ROWS
    cap = 1 if planes >= 2048 else 2048 // planes
    return min(want, cap)


class Memory:
    """a flat byte buffer with one array at byte address `base`: loads and stores are checked against its extent"""

    def __init__(self, data, base, elem):
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.base, self.size, self.elem = base, raw.size, elem
        self.buf = np.full(base + raw.size + 16, 0xEE, np.uint8)
        self.buf[base:base + raw.size] = raw
        self.wide = self.narrow = 0

    def _check(self, addr, nbytes, aligned_to):
        assert self.base <= addr and addr + nbytes <= self.base + self.size, (addr, nbytes, self.base, self.size)
        assert addr % aligned_to == 0, (addr, aligned_to)
        if nbytes > self.elem:
            self.wide += 1
        else:
            self.narrow += 1

    def load(self, addr, nbytes, aligned_to=1):
        self._check(addr, nbytes, aligned_to)
        return self.buf[addr:addr + nbytes].tobytes()

    def store(self, addr, data, aligned_to=1):
        self._check(addr, len(data), aligned_to)
        self.buf[addr:addr + len(data)] = np.frombuffer(data, np.uint8)

    def array(self, dtype, shape):
        return self.buf[self.base:self.base + self.size].view(dtype).reshape(shape).copy()


def ingest_window_transcription(x, y0, x0, wh, ww, H, W, mode, kind, base=0, grid_x=None):
    """csrc/ingest_pad.hip's kernels, given a window, on frames x (layout `kind`) at byte address `base` -> (out float32 (F, C, H, W), wide loads,
    narrow loads); the output is taken as 16-byte aligned, which the entry point requires"""
    x = np.ascontiguousarray(x)
    edge = mode == "edge"
    assert mode in ("reflect", "edge")
    if kind == U8_INTERLEAVED:
        F, h, w, C = x.shape
        assert C == 3
    else:
        F, C, h, w = x.shape
    assert 0 <= y0 and 0 <= x0 and 1 <= wh <= h - y0 and 1 <= ww <= w - x0 and H >= wh and W >= ww
    elem = 4 if kind == F32_PLANES else 1
    assert base % elem == 0
    mem = Memory(x, base, elem)
    out = np.zeros(F * C * H * W, np.uint32)
    stored = np.zeros(F * C * H * W, np.int32)
    vec = W % 4 == 0
    cols = W // 4 if vec else W

    def unit(v):
        return (F32(v) / F32(255)).view(np.uint32)

    def store(at, words):
        assert 0 <= at and at + len(words) <= out.size and (len(words) == 1 or (len(words) == 4 and (4 * at) % 16 == 0))
        out[at:at + len(words)] = words
        stored[at:at + len(words)] += 1

    def word(addr):
        if addr % 4 == 0:
            return int.from_bytes(mem.load(addr, 4, 4), "little")
        return sum(mem.load(addr + j, 1)[0] << (8 * j) for j in range(4))

    px = 3 if kind == U8_INTERLEAVED else 1      # samples per pixel step along a row
    planes = F if kind == U8_INTERLEAVED else F * C
    gx = row_blocks(H, planes) if grid_x is None else grid_x
    grid = [(bx, c, f) for f in range(F) for c in range(1 if kind == U8_INTERLEAVED else C) for bx in range(gx)]
    for bx, by, bz in grid:
        plane = bz if kind == U8_INTERLEAVED else bz * C + by
        src = base + (plane * h * w * px + x0 * px) * elem
        dst = plane * H * W * px
        for ty in range(ROWS):
            y = bx * ROWS + ty
            while y < H:
                row = src + (y0 + src_index(y, wh, edge)) * w * px * elem
                for xv in range(cols):      # lane xv % 64, pass xv // 64
                    if not vec:
                        at = row + src_index(xv, ww, edge) * px * elem
                        if kind == U8_INTERLEAVED:
                            for c in range(3):
                                store(dst + c * H * W + y * W + xv, [unit(mem.load(at + c, 1)[0])])
                        else:
                            v = mem.load(at, elem, elem)
                            store(dst + y * W + xv, [unit(v[0]) if elem == 1 else int.from_bytes(v, "little")])
                        continue
                    xq = 4 * xv
                    straight = xq + 4 <= ww
                    p = row + xq * px * elem
                    if kind == U8_INTERLEAVED:
                        if straight:
                            twelve = b"".join(word(p + 4 * k).to_bytes(4, "little") for k in range(3))
                        else:
                            twelve = b"".join(mem.load(row + src_index(xq + j, ww, edge) * 3 + c, 1) for j in range(4) for c in range(3))
                        for c in range(3):
                            store(dst + c * H * W + y * W + xq, [unit(twelve[3 * j + c]) for j in range(4)])
                    elif elem == 1:
                        if straight:
                            wd = word(p)
                        else:
                            wd = sum(mem.load(row + src_index(xq + j, ww, edge), 1)[0] << (8 * j) for j in range(4))
                        store(dst + y * W + xq, [unit((wd >> (8 * j)) & 255) for j in range(4)])
                    else:
                        if straight and p % 16 == 0:
                            q = mem.load(p, 16, 16)
                        elif straight:
                            q = b"".join(mem.load(p + 4 * j, 4, 4) for j in range(4))
                        else:
                            q = b"".join(mem.load(row + src_index(xq + j, ww, edge) * 4, 4, 4) for j in range(4))
                        store(dst + y * W + xq, [int.from_bytes(q[4 * j:4 * j + 4], "little") for j in range(4)])
                y += gx * ROWS
    assert (stored == 1).all(), "every output sample is stored exactly once"
    return out.view(F32).reshape(F, C, H, W), mem.wide, mem.narrow


def tile_blend_transcription(acc, sr_store, sr_offset, sr_shape, sr_strides, Y0, X0, wy, wx, bases=(0, 0, 0, 0), grid_x=None):
    """csrc/blend.hip's rows kernel with both flips off: `ensemble_ref.blend_dihedral_transcription` at k = 0 (which see; that module
    imports this one, hence the import here)"""
    from tests.ensemble_ref import blend_dihedral_transcription
    return blend_dihedral_transcription(acc, sr_store, sr_offset, sr_shape, sr_strides, 0, Y0, X0, wy, wx, bases=bases, grid_x=grid_x)
