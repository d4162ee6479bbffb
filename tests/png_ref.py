"""An independent numpy / pure-Python oracle for the device PNG encoder (csrc/png.hip): the five scanline filters with libpng's default
row heuristic, and an inflate-side parser that walks a zlib stream block by block and reports what it is made of.  No GPU, nothing
from eavsr_amd; zlib itself is the judge of validity (`zlib.decompress` checks the Adler-32), the parser only describes."""
import struct
import zlib

import numpy as np

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ------------------------------------------------------------------------------------------------------------------- filters
def filter_candidates(img):
    """img (H, W, C) uint8 -> (5, H, W C) uint8: every row under filters 0 - 4 (PNG specification 9.2).  Neighbours outside the image
    are 0; every filter reads original pixels."""
    img = np.asarray(img, np.uint8)
    h, w, c = img.shape
    x = img.reshape(h, w * c).astype(np.int32)
    a = np.zeros_like(x)
    a[:, c:] = x[:, :-c]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, c:] = x[:-1, :-c]
    p = a + b - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)


def row_costs(cand):
    """(5, H, R) filtered rows -> (5, H) int64: the sum over a row of |byte read as signed|"""
    return np.abs(cand.astype(np.int8).astype(np.int64)).sum(2)


def choose_filters(costs):
    """the smallest cost wins, a tie goes to the lowest filter number (np.argmin returns the first minimum)"""
    return np.argmin(costs, axis=0)


def filter_rows(img, types=None):
    """img (H, W, C) uint8 -> (H, 1 + W C) uint8 scanlines, byte 0 the filter type: chosen by the heuristic, or `types` (an int or one
    per row) forced"""
    cand = filter_candidates(img)
    h = cand.shape[1]
    ft = choose_filters(row_costs(cand)) if types is None else np.broadcast_to(np.asarray(types), (h,))
    rows = cand[ft, np.arange(h)]
    return np.concatenate([ft.astype(np.uint8)[:, None], rows], 1)


def filter_frames(frames):
    """(F, H, W, C) -> (F, H, 1 + W C): frames are independent"""
    return np.stack([filter_rows(f) for f in np.asarray(frames, np.uint8)])


# --------------------------------------------------------------------------------------------------------------------- files
def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_file(idat, h, w, c):
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0)) + chunk(b"IDAT", idat)
            + chunk(b"IEND", b""))


def split_png(data):
    """a PNG file -> ((w, h, depth, colour type, compression, filter, interlace), [IDAT bodies]); every chunk CRC is checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, hdr, idat, tags = 8, None, [], []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert zlib.crc32(tag + body) & 0xFFFFFFFF == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0], tag
        tags.append(tag)
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        if tag == b"IDAT":
            idat.append(body)
        pos += 12 + n
    assert pos == len(data) and tags[0] == b"IHDR" and tags[-1] == b"IEND"
    return hdr, idat


def inflate_all(stream):
    """zlib.decompress that also insists the stream is consumed to its last byte (zlib then has verified the Adler-32)"""
    d = zlib.decompressobj()
    out = d.decompress(stream)
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", "the zlib stream does not end where the buffer ends"
    return out


def huffman_only_stripes(raw, stripe_bytes):
    """zlib's own Huffman-only coder framed as the device coder frames a stream: every stripe one raw-deflate
    compressobj(1, DEFLATED, -15, 9, Z_HUFFMAN_ONLY) ended by Z_SYNC_FLUSH, between 78 01 and 03 00 + Adler-32"""
    out = [b"\x78\x01"]
    for first in range(0, len(raw), stripe_bytes):
        c = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        out.append(c.compress(raw[first:first + stripe_bytes]) + c.flush(zlib.Z_SYNC_FLUSH))
    out.append(b"\x03\x00" + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF))
    return b"".join(out)


# -------------------------------------------------------------------------------------------------------------------- parser
class _Bits:
    def __init__(self, data, pos=0):
        self.data, self.pos = data, pos      # pos in bits

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7


def _decoder(lengths):
    """{(length, code): symbol} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for sym, n in enumerate(lengths):
        if n:
            table[(n, nxt[n])] = sym
            nxt[n] += 1
    return table


def _symbol(bits, table):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | bits.take(1)      # Huffman codes are packed most significant bit first
        if (n, code) in table:
            return table[(n, code)]
    raise ValueError("no code of up to 15 bits matches")


def kraft(lengths):
    return sum(2.0 ** -n for n in lengths if n)


def parse_zlib(stream):
    """Walk a zlib stream.  Returns {'blocks': [...], 'data': bytes, 'adler_ok': bool, 'consumed': bytes used}; a block is
    {'type': 'stored' | 'fixed' | 'dynamic', 'final': bool, 'bytes': output bytes, 'has_match': a length / distance symbol occurred}
    and for a dynamic block also 'lit_lengths' (HLIT + 257 values), 'dist_lengths', 'cl_lengths' (19, in symbol order)."""
    cmf, flg = stream[0], stream[1]
    assert cmf & 15 == 8 and (cmf * 256 + flg) % 31 == 0 and not flg & 32, "zlib header"
    bits = _Bits(stream, 16)
    out = bytearray()
    blocks = []
    LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
    DEXT = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
    while True:
        final, btype = bits.take(1), bits.take(2)
        blk = {"final": bool(final), "has_match": False}
        start = len(out)
        if btype == 0:
            bits.align()
            n, nn = bits.take(16), bits.take(16)
            assert n ^ nn == 0xFFFF, "stored block: LEN / NLEN"
            out += stream[bits.pos >> 3:(bits.pos >> 3) + n]
            bits.pos += 8 * n
            blk["type"] = "stored"
        elif btype in (1, 2):
            if btype == 1:
                lit = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dist = [5] * 30
                blk["type"] = "fixed"
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits.take(3)
                cltab = _decoder(cl)
                seq = []
                while len(seq) < hlit + hdist:
                    s = _symbol(bits, cltab)
                    if s < 16:
                        seq.append(s)
                    elif s == 16:
                        seq += [seq[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        seq += [0] * (3 + bits.take(3))
                    else:
                        seq += [0] * (11 + bits.take(7))
                assert len(seq) == hlit + hdist, "a run crosses the end of the code lengths"
                lit, dist = seq[:hlit], seq[hlit:]
                blk.update(type="dynamic", lit_lengths=lit, dist_lengths=dist, cl_lengths=cl)
            littab, disttab = _decoder(lit), _decoder(dist)
            while True:
                s = _symbol(bits, littab)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    blk["has_match"] = True
                    length = LBASE[s - 257] + bits.take(LEXT[s - 257])
                    d = _symbol(bits, disttab)
                    distance = DBASE[d] + bits.take(DEXT[d])
                    for _ in range(length):
                        out.append(out[-distance])
        else:
            raise ValueError("block type 3")
        blk["bytes"] = len(out) - start
        blocks.append(blk)
        if final:
            break
    bits.align()
    at = bits.pos >> 3
    adler = struct.unpack(">I", stream[at:at + 4])[0]
    return {"blocks": blocks, "data": bytes(out), "adler_ok": adler == (zlib.adler32(bytes(out)) & 0xFFFFFFFF), "consumed": at + 4}
