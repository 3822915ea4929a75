// bwt_dev.hpp — device-side pieces that more than one of the suffix sort's kernel files share (bwt_round1.hip, bwt_tile_sort.hip,
// bwt_defer.hip, bwt_regroup.hip; the map is in bwt.hip): the block geometries, the block of a sorted position without a division,
// the flag and head bytes as 16-slot masks, two wave-wide searches for a group head, and the eight text bytes around a suffix.
// The rules themselves are in bwt_rules.h.
#pragma once
#include "bwt_parts.h"      // (and radix.hpp, prims.hpp, bwt_rules.h through it)
#include <type_traits>

namespace cjs {

__device__ __forceinline__ uint32_t blk_len(const Geom& g, uint32_t blk) { return blk == g.nb - 1 ? g.n_last : g.stride; }
__device__ __forceinline__ uint32_t blk_len(const VarGeom& g, uint32_t blk) { return g.len[blk]; }

// Block of sorted position p without a division: pos[] ascends along the array, so a thread divides once, for its first slot, and
// steps from the block `prev` of a position at or below p (the same block or the next one; a tail round's window may span more)
__device__ __forceinline__ uint32_t blk_step(uint32_t p, uint32_t stride, uint32_t prev) {
  const uint32_t off = p - prev * stride;
  return off < stride ? prev : off - stride < stride ? prev + 1u : p / stride;
}

// bit `bit` of each of the 16 flag bytes in v -> 16-bit mask (byte j -> bit j)
__device__ __forceinline__ uint32_t hf_bits16(const uint4& v, int bit) {
  return hf_bits4(v.x, bit) | (hf_bits4(v.y, bit) << 4) | (hf_bits4(v.z, bit) << 8) | (hf_bits4(v.w, bit) << 12);
}
// the 16 flag bytes of slots [base + 16 * tid, +16) of a tile (tile bases and hflag are 16-byte aligned; chunks that start at or
// past A are not read) and the mask of those slots that lie below A
__device__ __forceinline__ uint4 hf_load16(const uint8_t* __restrict__ hflag, uint64_t base, uint32_t nvalid, int tid, uint32_t& valid) {
  const uint32_t first = (uint32_t)tid * 16u;
  const uint32_t nv = nvalid > first ? (nvalid - first < 16u ? nvalid - first : 16u) : 0u;
  valid = (1u << nv) - 1u;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (nv) v = *reinterpret_cast<const uint4*>(hflag + base + first);
  return v;
}

// The shared wave idiom.  One lane per 64-slot mask word m of a 4096-slot tile or window (all 64 lanes): slot + 1 of the last
// head strictly before this lane's word, 0 = none; incl = the same with this word counted in.
__device__ __forceinline__ uint32_t last_head_before_word(uint64_t m, int lane, uint32_t& incl) {
  const uint32_t lastrel = m ? (uint32_t)lane * 64u + 63u - (uint32_t)__builtin_clzll(m) + 1u : 0u;
  incl = wave_incl_max(lastrel);
  uint32_t em = __shfl_up(incl, 1, 64);
  if (lane == 0) em = 0;
  return em;
}

// Wave-uniform: global index of the first slot of the class that runs into slot `base` from the left, inside [seg0, base] (the
// block is sorted by class, seg0 = its first slot); class_at(i) = the class key of slot i.  Looks at the 64 slots in front of
// `base` -- nearly always enough -- and otherwise makes a 64-way search for the lower bound of the class in the block.  Needs all
// 64 lanes.
template <typename ClassAt>
__device__ __forceinline__ uint64_t class_head_before_by(ClassAt class_at, uint64_t seg0, uint64_t base, int lane) {
  if (base == seg0) return base;
  const uint64_t target = class_at(base);
  const uint64_t off = base - seg0;
  const uint32_t back = off < 64u ? (uint32_t)off : 64u;                // slots in front of base, inside the block
  const bool eq = (uint32_t)lane < back && class_at(base - 1u - (uint32_t)lane) == target;
  const uint64_t ne = ~__ballot(eq);
  const uint32_t m = ne ? (uint32_t)__builtin_ctzll(ne) : 64u;          // slots base-1 .. base-m carry the class
  if (m < 64u || off <= 64u) return base - m;
  uint64_t lo = seg0, hi = base - 64u;                                  // slot hi is known to carry the class
  while (hi > lo) {
    const uint64_t len = hi - lo, step = (len + 63u) / 64u, idx = lo + (uint64_t)lane * step;
    const bool hit = idx >= hi || class_at(idx) == target;
    const uint64_t hits = __ballot(hit);
    const uint32_t j = hits ? (uint32_t)__builtin_ctzll(hits) : 64u;    // first probe inside the class (64: none, it starts behind the last probe)
    if (!j) { hi = lo; break; }
    const uint64_t nhi = lo + (uint64_t)j * step;
    lo += (uint64_t)(j - 1u) * step + 1u;
    if (j < 64u && nhi < hi) hi = nhi;
  }
  return hi;
}
// ... with the class of a slot = its key >> shift
__device__ __forceinline__ uint64_t class_head_before(const uint64_t* __restrict__ key, uint64_t seg0, uint64_t base, int shift, int lane) {
  return class_head_before_by([&](uint64_t i) { return key[i] >> shift; }, seg0, base, lane);
}

// The eight text bytes around position p of a cyclic block of n bytes at tx: byte j of the result = tx[(p - 1 + j) mod n].
// text8_words: three aligned 32-bit loads from the aligned-down ABSOLUTE address (block rows start at odd addresses) + alignbyte;
// every load address is clamped to the words that hold a byte of the block, so it is safe for every p < n, and right for
// 1 <= p, p + 6 < n.  The other positions wrap: text8_wrapping steps byte by byte (a block shorter than 7 bytes wraps more
// than once).
__device__ __forceinline__ bool text8_wraps(uint32_t p, uint32_t n) { return p == 0 || p + 6 >= n; }
__device__ __forceinline__ uint64_t text8_words(const uint8_t* __restrict__ tx, uint32_t p, uint32_t n) {
  const uint32_t t0 = (uint32_t)((uintptr_t)tx & 3u);
  const uint8_t* txa = tx - t0;
  const int last = (int)((t0 + n - 1u) & ~3u);                  // byte offset of the last word that holds a byte of the block
  const int q = (int)(t0 + p) - 1, o = q & ~3;
  const uint32_t sh = (uint32_t)q & 3u;
  auto word = [&](int at) { return *reinterpret_cast<const uint32_t*>(txa + (at < 0 ? 0 : at > last ? last : at)); };
  const uint32_t a0 = word(o), a1 = word(o + 4), a2 = word(o + 8);
  return ((uint64_t)__builtin_amdgcn_alignbyte(a2, a1, sh) << 32) | __builtin_amdgcn_alignbyte(a1, a0, sh);
}
__device__ __forceinline__ uint64_t text8_wrapping(const uint8_t* __restrict__ tx, uint32_t p, uint32_t n) {
  uint32_t x = p ? p - 1u : n - 1u;
  uint64_t t = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) { t |= (uint64_t)tx[x] << (8 * j); x = x + 1u == n ? 0u : x + 1u; }
  return t;
}
__device__ __forceinline__ uint64_t text8(const uint8_t* __restrict__ tx, uint32_t p, uint32_t n) {
  return text8_wraps(p, n) ? text8_wrapping(tx, p, n) : text8_words(tx, p, n);
}

}  // namespace cjs
