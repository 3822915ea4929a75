// crc32_bz.h — the arithmetic of the bzip2 CRC-32 (MSB-first, poly 0x04c11db7, init ~0, final ~) as crc.hip computes it in
// pieces.  No HIP: plain constexpr functions that the kernels and the host compiler read alike (tests/host/rle1_rules_check.cc
// checks them against a bit-by-bit CRC).
// The CRC register after a string is linear in the string: CRC0(A|B) = CRC0(A) * x^(8|B|) + CRC0(B) in GF(2)[x]/P
// (CRC0 = zero initial value).  A range is cut at 16 KiB-aligned ADDRESS windows, every window into 64-byte pieces; a piece's
// CRC0 is multiplied by x^(8 * bytes behind it) and the products are XORed.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cjs {

constexpr uint32_t CRC_POLY = 0x04c11db7u;
constexpr uint32_t CRC_SEG = 16384;   // bytes per window: 256 pieces of 64 bytes

constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {                           // a*b mod P, bit k = x^k
  uint32_t r = 0;
#if defined(__clang__)
#pragma unroll 4
#endif
  for (int i = 31; i >= 0; i--) {
    r = (r << 1) ^ ((r & 0x80000000u) ? CRC_POLY : 0u);
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}
constexpr uint32_t gf_xpow8(uint64_t nbytes) {                                // x^(8*nbytes) mod P, by squaring
  uint32_t result = 1u, base = 0x100u;                                        // x^8
  while (nbytes) {
    if (nbytes & 1) result = gf_mul(result, base);
    base = gf_mul(base, base);
    nbytes >>= 1;
  }
  return result;
}

struct CrcTables {
  uint32_t tab[4][256];    // slicing-by-4: tab[k][i] = CRC0 of byte i followed by k zero bytes
  uint32_t pw64[256];      // x^(8*64*q)
  uint32_t px[64];         // x^(8*r)
};
constexpr CrcTables make_crc_tables() {
  CrcTables t{};
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i << 24;
    for (int k = 0; k < 8; k++) c = (c & 0x80000000u) ? (c << 1) ^ CRC_POLY : (c << 1);
    t.tab[0][i] = c;
  }
  for (int k = 1; k < 4; k++)
    for (uint32_t i = 0; i < 256; i++) { const uint32_t p = t.tab[k - 1][i]; t.tab[k][i] = (p << 8) ^ t.tab[0][p >> 24]; }
  t.px[0] = 1u;
  for (int r = 1; r < 64; r++) t.px[r] = gf_mul(t.px[r - 1], 0x100u);
  const uint32_t x64 = gf_mul(t.px[63], 0x100u);
  t.pw64[0] = 1u;
  for (int q = 1; q < 256; q++) t.pw64[q] = gf_mul(t.pw64[q - 1], x64);
  return t;
}
// x^(8*n) for n < CRC_SEG from the tables
constexpr uint32_t gf_xpow8_small(uint32_t n, const uint32_t* pw64, const uint32_t* px) {
  const uint32_t q = n >> 6, r = n & 63u;
  return r ? gf_mul(pw64[q], px[r]) : pw64[q];
}

// Window i of the byte range [s, e) of the address space: W = the window's first address (windows are aligned, so that every
// 16-byte load of a window is an aligned one), [lo, hi) = the bytes of the range in it.  The range's windows are those with W < e.
struct CrcWindow { uint64_t W, lo, hi; };
constexpr CrcWindow crc_window(uint64_t s, uint64_t e, uint32_t i) {
  const uint64_t W = (s & ~(uint64_t)(CRC_SEG - 1)) + (uint64_t)i * CRC_SEG;
  return {W, W > s ? W : s, W + CRC_SEG < e ? W + CRC_SEG : e};
}
// bound on the windows that a range of len bytes touches, wherever it starts (the partial CRCs of a range take this many words)
constexpr size_t crc_segs_for(size_t len) { return (len + CRC_SEG - 1) / CRC_SEG + 1; }

}  // namespace cjs
