// The serial part of a literal-only dynamic-Huffman deflate block (RFC 1951, BTYPE = 10): code lengths limited to 15 bits, canonical
// codes, and the block header with its run-length coded lengths and the 7-bit code-length alphabet.  A few thousand operations per
// block; csrc/png.hip runs them on one lane per stripe with every array in LDS.  The functions are plain C++ on plain pointers
// (EAVSR_HD), so a host program can compile this file as it is and check the tables against zlib's inflate without a device.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define EAVSR_HD __host__ __device__ __forceinline__
#else
#define EAVSR_HD inline
#endif

namespace eavsr_deflate {

constexpr int kLit = 257;            // 256 literals + end-of-block: no length symbol is ever sent (HLIT = 0)
constexpr int kSeq = kLit + 1;       // + the one distance code of zero bits (HDIST = 0; RFC 1951 3.2.7: all-literal data)
constexpr int kCl = 19;              // the code-length alphabet
constexpr int kMaxHeaderBits = 17 + 3 * kCl + 14 * kSeq;      // loose: every entry 7 code bits + 7 extra bits

// OR the low `n` bits of v into a zeroed little-endian bit buffer of 64-bit words (deflate packs from the least significant bit)
EAVSR_HD void put_bits(uint64_t* buf, uint32_t& pos, uint32_t v, int n) {
  if (n == 0) return;
  const uint32_t sh = pos & 63;
  buf[pos >> 6] |= (uint64_t)v << sh;
  if (sh + (uint32_t)n > 64) buf[(pos >> 6) + 1] |= (uint64_t)v >> (64 - sh);
  pos += (uint32_t)n;
}

EAVSR_HD uint32_t reverse_bits(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

// Code lengths of a Huffman code limited to `maxbits`.  sorted[0 .. n): the symbols of non-zero frequency in ascending (frequency,
// symbol) order, n >= 1; lens[] is zero on entry for every symbol.  Scratch: w[2 n], par[2 n].
//   1. the Huffman tree by the two-queue method (leaves in sorted order, internal nodes in the order they are made);
//   2. depths from the root down, clamped to maxbits at every node; `overflow` counts the nodes, internal ones included, that were;
//   3. zlib's repair (trees.c gen_bitlen): while overflow > 0, one leaf of the deepest level above maxbits becomes an internal
//      node whose two children are itself and one leaf taken from maxbits; overflow falls by 2 -- the Kraft sum ends at exactly 1;
//   4. lengths are handed out by count, longest to the rarest symbol.
EAVSR_HD void build_lengths(const uint32_t* freq, const uint16_t* sorted, int n, int maxbits, uint8_t* lens, uint32_t* w, uint16_t* par) {
  if (n == 1) {
    lens[sorted[0]] = 1;
    return;
  }
  for (int i = 0; i < n; ++i) w[i] = freq[sorted[i]];
  int leaf = 0, inode = n, next = n;
  for (int k = 0; k < n - 1; ++k) {
    int pick[2];
    for (int j = 0; j < 2; ++j) {
      const bool take_leaf = leaf < n && (inode >= next || w[leaf] <= w[inode]);
      pick[j] = take_leaf ? leaf++ : inode++;
    }
    w[next] = w[pick[0]] + w[pick[1]];
    par[pick[0]] = par[pick[1]] = (uint16_t)next;
    ++next;
  }
  int count[16];
  for (int b = 0; b < 16; ++b) count[b] = 0;
  int overflow = 0;
  w[2 * n - 2] = 0;      // the weights are spent: w[] now holds depths, parents (higher indices) before children
  for (int i = 2 * n - 3; i >= 0; --i) {
    int d = (int)w[par[i]] + 1;
    if (d > maxbits) d = maxbits, ++overflow;      // internal nodes count too, and hand the CLAMPED depth down (as gen_bitlen does)
    w[i] = (uint32_t)d;
    if (i < n) ++count[d];
  }
  while (overflow > 0) {
    int bits = maxbits - 1;
    while (count[bits] == 0) --bits;
    --count[bits];
    count[bits + 1] += 2;
    --count[maxbits];
    overflow -= 2;
  }
  int i = 0;
  for (int bits = maxbits; bits >= 1; --bits)
    for (int c = 0; c < count[bits]; ++c) lens[sorted[i++]] = (uint8_t)bits;
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for the LSB-first stream: tab[s] = len << 16 | reversed code
EAVSR_HD void canonical_codes(const uint8_t* lens, int nsym, uint32_t* tab) {
  int count[16], next[16];
  for (int b = 0; b < 16; ++b) count[b] = 0;
  for (int s = 0; s < nsym; ++s) ++count[lens[s]];
  count[0] = 0;
  int code = 0;
  next[0] = 0;
  for (int b = 1; b < 16; ++b) {
    code = (code + count[b - 1]) << 1;
    next[b] = code;
  }
  for (int s = 0; s < nsym; ++s) {
    const int len = lens[s];
    tab[s] = len ? ((uint32_t)len << 16) | reverse_bits((uint32_t)next[len]++, len) : 0u;
  }
}

// The block header into buf (zeroed) from bit `pos` on: BFINAL = 0, BTYPE = 10, HLIT = 0, HDIST = 0, HCLEN, the code-length code
// lengths, then lens[0 .. 257) and the one distance length 0 as symbols 0 - 15 / 16 (repeat 3 - 6) / 17 (3 - 10 zeros) / 18 (11 - 138
// zeros).  Scratch: rle[kSeq] (symbol | extra value << 5), w[2 kCl], par[2 kCl].
EAVSR_HD void write_header(const uint8_t* lens, uint64_t* buf, uint32_t& pos, uint16_t* rle, uint32_t* w, uint16_t* par) {
  int nrle = 0;
  uint32_t clfreq[kCl];
  for (int s = 0; s < kCl; ++s) clfreq[s] = 0;
  auto emit = [&](int sym, int extra) {
    rle[nrle++] = (uint16_t)(sym | (extra << 5));
    ++clfreq[sym];
  };
  auto at = [&](int i) { return i < kLit ? (int)lens[i] : 0; };
  for (int i = 0; i < kSeq;) {
    const int v = at(i);
    int run = 1;
    while (i + run < kSeq && at(i + run) == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int r = run < 138 ? run : 138;
        emit(18, r - 11);
        run -= r;
      }
      if (run >= 3) emit(17, run - 3), run = 0;
    } else {
      emit(v, 0);
      --run;
      while (run >= 3) {
        const int r = run < 6 ? run : 6;
        emit(16, r - 3);
        run -= r;
      }
    }
    for (; run > 0; --run) emit(v, 0);
  }
  uint16_t order[kCl];
  int nused = 0;
  for (int s = 0; s < kCl; ++s) {      // insertion sort by (frequency, symbol)
    if (clfreq[s] == 0) continue;
    int j = nused++;
    for (; j > 0 && clfreq[order[j - 1]] > clfreq[s]; --j) order[j] = order[j - 1];
    order[j] = (uint16_t)s;
  }
  uint8_t cllen[kCl];
  uint32_t cltab[kCl];
  for (int s = 0; s < kCl; ++s) cllen[s] = 0;
  build_lengths(clfreq, order, nused, 7, cllen, w, par);
  canonical_codes(cllen, kCl, cltab);
  const uint8_t perm[kCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int ncl = kCl;
  while (ncl > 4 && cllen[perm[ncl - 1]] == 0) --ncl;
  put_bits(buf, pos, 0, 1);
  put_bits(buf, pos, 2, 2);
  put_bits(buf, pos, 0, 5);
  put_bits(buf, pos, 0, 5);
  put_bits(buf, pos, (uint32_t)(ncl - 4), 4);
  for (int k = 0; k < ncl; ++k) put_bits(buf, pos, cllen[perm[k]], 3);
  for (int k = 0; k < nrle; ++k) {
    const int sym = rle[k] & 31, extra = rle[k] >> 5;
    put_bits(buf, pos, cltab[sym] & 0xffff, (int)(cltab[sym] >> 16));
    if (sym == 16) put_bits(buf, pos, (uint32_t)extra, 2);
    if (sym == 17) put_bits(buf, pos, (uint32_t)extra, 3);
    if (sym == 18) put_bits(buf, pos, (uint32_t)extra, 7);
  }
}

}  // namespace eavsr_deflate
