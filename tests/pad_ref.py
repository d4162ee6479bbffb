"""The padded ingest (ops.ingest_pad, csrc/ingest_pad.hip) restated twice with scalar numpy, nothing of eavsr_amd imported.

`pad_oracle`: the definition -- np.pad at the bottom and right, then `np.float32(v) / 255` for bytes (fp32 samples are kept).

`kernel_transcription`: the kernels' own address arithmetic, workgroup by workgroup and lane by lane, on a flat byte buffer with
the source at a byte offset: the grid (row groups x channel x frame), one wave per output row, a lane per quad of 4 output samples
(W % 4 == 0) or per sample, the "straight" test 4 xq + 4 <= w, the aligned 32-bit (fp32: 16-byte) load against the per-sample loads,
the triangle wave.  Every load asserts that it lies inside the source and, for a wide load, that its address is aligned; every
store asserts that it lies inside the output, is aligned and is the only store to its samples."""
import numpy as np

F32 = np.float32
LANES, ROWS = 64, 4
U8_PLANES, U8_INTERLEAVED, F32_PLANES = 0, 1, 2


def pad_oracle(x: np.ndarray, H: int, W: int, mode: str, hwc: bool = False) -> np.ndarray:
    """x uint8 / float32 (F, C, h, w), or uint8 (F, h, w, 3) with hwc -> float32 (F, C, H, W)"""
    x = np.asarray(x)
    if hwc:
        x = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    h, w = x.shape[-2:]
    padded = np.pad(x, ((0, 0), (0, 0), (0, H - h), (0, W - w)), mode=mode)
    if x.dtype == np.uint8:
        return padded.astype(F32) / F32(255)
    return padded


def src_index(i: int, s: int, edge: bool) -> int:
    """csrc/ingest_pad.hip `src_index`, in 32-bit unsigned arithmetic"""
    assert 0 <= i < 2 ** 32 and 1 <= s < 2 ** 31
    if i < s:
        return i
    if edge or s == 1:
        return s - 1
    period = 2 * (s - 1)
    assert period < 2 ** 32
    m = i % period
    return m if m < s else period - m


def row_blocks(H: int, planes: int) -> int:
    want = (H + ROWS - 1) // ROWS
    cap = 1 if planes >= 2048 else 2048 // planes
    return min(want, cap)


class _Memory:
    """a flat byte buffer with the source at `base`: loads are checked against the source's extent"""

    def __init__(self, data: np.ndarray, base: int, elem: int):
        self.elem = elem
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.base, self.size = base, raw.size
        self.buf = np.zeros(base + raw.size + 16, np.uint8)
        self.buf[:base] = 0xEE
        self.buf[base + raw.size:] = 0xEE
        self.buf[base:base + raw.size] = raw
        self.wide = self.narrow = 0

    def load(self, addr: int, nbytes: int, aligned_to: int = 1) -> bytes:
        assert self.base <= addr and addr + nbytes <= self.base + self.size, (addr, nbytes, self.base, self.size)
        assert addr % aligned_to == 0, (addr, aligned_to)
        if nbytes > self.elem:      # one load of several samples
            self.wide += 1
        else:
            self.narrow += 1
        return self.buf[addr:addr + nbytes].tobytes()


def kernel_transcription(x: np.ndarray, H: int, W: int, mode: str, kind: int, base: int = 0, grid_x=None):
    """x as `pad_oracle` takes it (kind names the layout) -> (out float32 (F, C, H, W), wide loads, narrow loads).  `base`: the byte
    address of the source's first byte (the output is taken as 16-byte aligned, which the entry point requires)."""
    x = np.ascontiguousarray(x)
    edge = mode == "edge"
    assert mode in ("reflect", "edge")
    if kind == U8_INTERLEAVED:
        F, h, w, C = x.shape
        assert C == 3
    else:
        F, C, h, w = x.shape
    assert H >= h and W >= w and F <= 65535 and C <= 65535
    elem = 4 if kind == F32_PLANES else 1
    mem = _Memory(x, base, elem)
    assert base % elem == 0
    out = np.zeros(F * C * H * W, np.uint32)      # the bit patterns
    stored = np.zeros(F * C * H * W, np.int32)
    vec = W % 4 == 0
    cols = W // 4 if vec else W

    def unit(v):
        return (F32(v) / F32(255)).view(np.uint32)

    def store(at, words):      # `at` in samples from the output's base
        assert 0 <= at and at + len(words) <= out.size
        assert len(words) == 1 or (len(words) == 4 and (4 * at) % 16 == 0)
        out[at:at + len(words)] = words
        stored[at:at + len(words)] += 1

    def word(addr):      # load_word of a byte source
        if addr % 4 == 0:
            return int.from_bytes(mem.load(addr, 4, 4), "little")
        return sum(mem.load(addr + j, 1)[0] << (8 * j) for j in range(4))

    if kind == U8_INTERLEAVED:
        gx = row_blocks(H, F) if grid_x is None else grid_x
        grid = [(bx, 0, f) for f in range(F) for bx in range(gx)]
    else:
        gx = row_blocks(H, F * C) if grid_x is None else grid_x
        grid = [(bx, c, f) for f in range(F) for c in range(C) for bx in range(gx)]
    for bx, by, bz in grid:
        for ty in range(ROWS):
            y = bx * ROWS + ty
            while y < H:
                ry = src_index(y, h, edge)
                for tx in range(min(LANES, cols)):
                    xv = tx
                    while xv < cols:
                        if kind == U8_INTERLEAVED:
                            src = base + bz * h * w * 3
                            row = src + ry * w * 3
                            dst = bz * H * W * 3 + y * W
                            if not vec:
                                px = row + src_index(xv, w, edge) * 3
                                for c in range(3):
                                    store(dst + c * H * W + xv, [unit(mem.load(px + c, 1)[0])])
                            else:
                                x0 = 4 * xv
                                if x0 + 4 <= w:
                                    p = row + x0 * 3
                                    twelve = b"".join(word(p + 4 * k).to_bytes(4, "little") for k in range(3))
                                else:
                                    twelve = b"".join(mem.load(row + src_index(x0 + j, w, edge) * 3 + c, 1) for j in range(4) for c in range(3))
                                for c in range(3):
                                    store(dst + c * H * W + x0, [unit(twelve[3 * j + c]) for j in range(4)])
                        else:
                            plane = bz * C + by
                            src = base + plane * h * w * elem
                            row = src + ry * w * elem
                            dst = plane * H * W + y * W
                            if not vec:
                                v = mem.load(row + src_index(xv, w, edge) * elem, elem, elem)
                                store(dst + xv, [unit(v[0]) if elem == 1 else int.from_bytes(v, "little")])
                            else:
                                x0 = 4 * xv
                                p = row + x0 * elem
                                straight = x0 + 4 <= w
                                if elem == 1:
                                    if straight:
                                        wd = word(p)
                                    else:
                                        wd = sum(mem.load(row + src_index(x0 + j, w, edge), 1)[0] << (8 * j) for j in range(4))
                                    store(dst + x0, [unit((wd >> (8 * j)) & 255) for j in range(4)])
                                else:
                                    if straight and p % 16 == 0:
                                        q = mem.load(p, 16, 16)
                                    elif straight:
                                        q = b"".join(mem.load(p + 4 * j, 4, 4) for j in range(4))
                                    else:
                                        q = b"".join(mem.load(row + src_index(x0 + j, w, edge) * 4, 4, 4) for j in range(4))
                                    store(dst + x0, [int.from_bytes(q[4 * j:4 * j + 4], "little") for j in range(4)])
                        xv += LANES
                y += gx * ROWS
    assert (stored == 1).all(), "every output sample is stored exactly once"
    return out.view(F32).reshape(F, C, H, W), mem.wide, mem.narrow
