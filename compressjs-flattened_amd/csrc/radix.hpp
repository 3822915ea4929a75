// radix.hpp — device-side pieces that the radix sorter (radix.hip) and the suffix-sort kernels (bwt_*.hip) share: the XCD tile
// order, the tile geometry of a segmented sort, the key source of round 1 (rs_hist and rs_scatter are instantiated on it; the
// record layouts are bwt_rules.h) and the wave ranking step of a scatter.
#pragma once
#include "cjs_internal.h"
#include "prims.hpp"
#include "bwt_rules.h"

namespace cjs {

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MiB L2),
// so workgroup w = 8*j + x works on tile x*ceil(T/8) + j: every XCD walks ONE contiguous range of the
// suffix array, i.e. one block at a time, and that block's rank array (3.6 MB) stays in its L2 while the
// kernel scatters / gathers ranks at random positions of it.  Speed only; any mapping is correct.
__device__ __forceinline__ uint32_t xcd_tile(uint32_t wg, uint32_t T) {
  const uint32_t per = (T + 7u) >> 3;
  return (wg & 7u) * per + (wg >> 3);
}
__host__ __device__ __forceinline__ uint32_t xcd_grid(uint32_t T) { return ((T + 7u) >> 3) << 3; }

// Segments: the array is nseg runs of `stride` elements (the last one n_last) that are sorted independently in the
// same launches (round 1 of the suffix sort: one segment per block, so the block id needs no digit passes of its
// own).  Tiles never straddle segments: segment s owns tiles [s*tps, (s+1)*tps).  A plain sort is one segment.
struct SegGeom { uint32_t nseg, stride, n_last, tps; };
struct TileRef { uint32_t seg, off, nvalid; uint64_t base; };
__device__ __forceinline__ TileRef tile_ref(const SegGeom& sg, uint32_t tile) {
  TileRef t;
  t.seg = tile / sg.tps;
  t.off = (tile - t.seg * sg.tps) * RS_TILE;
  const uint32_t sn = t.seg + 1 == sg.nseg ? sg.n_last : sg.stride;
  t.nvalid = t.off < sn ? (sn - t.off < RS_TILE ? sn - t.off : RS_TILE) : 0u;
  t.base = (uint64_t)t.seg * sg.stride + t.off;
  return t;
}
// Key source of the first pass of round 1: keys are made on the fly from the block bytes (no key array is ever
// written for them).  key = leading nsym symbols | block parity above them (adjacent blocks must not compare equal);
// cyclic: bytes, wrapping; sentinel: 9-bit symbols byte+1, 0 = past the end.  value = position in the block.
// (the packed records of the cyclic round 1, packed == 2: pk_record of bwt_rules.h)
struct GenSrc { const uint8_t* T; int cyclic, nsym, packed; };
constexpr uint32_t GEN_PAD = 8;
// stages the tile's bytes (+GEN_PAD lookahead) in LDS; returns the byte offset of the tile's first byte inside tb (< 4):
// tiles that do not touch the end of their block are copied as aligned 32-bit words from the aligned-down address
__device__ __forceinline__ uint32_t gen_stage(const GenSrc& gs, const SegGeom& sg, const TileRef& t, uint8_t* tb) {
  const uint32_t sn = t.seg + 1 == sg.nseg ? sg.n_last : sg.stride;
  const uint8_t* src = gs.T + (size_t)t.seg * sg.stride;
  if (t.off + RS_TILE + GEN_PAD <= sn) {
    const uintptr_t a = (uintptr_t)(src + t.off);
    const uint32_t* al = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
    uint32_t* tw = reinterpret_cast<uint32_t*>(tb);
    for (uint32_t i = threadIdx.x; i < (RS_TILE + GEN_PAD) / 4 + 1; i += 256) tw[i] = al[i];
    return (uint32_t)(a & 3);
  }
  for (uint32_t i = threadIdx.x; i < RS_TILE + GEN_PAD; i += 256) {
    uint32_t p = t.off + i;
    if (p >= sn) p = gs.cyclic ? p % sn : sn - 1;      // sentinel: never used (masked by position)
    tb[i] = t.nvalid ? src[p] : 0;
  }
  return 0;
}
__device__ __forceinline__ uint64_t gen_key(const GenSrc& gs, const SegGeom& sg, const TileRef& t, const uint8_t* tb, uint32_t tb0, uint32_t loc) {
  // the 8 bytes at tb[tb0 + loc ..] from three aligned LDS words
  const uint32_t* tw = reinterpret_cast<const uint32_t*>(tb) + ((tb0 + loc) >> 2);
  const uint32_t a0 = tw[0], a1 = tw[1], a2 = tw[2], sh = (tb0 + loc) & 3u;
  const uint32_t lo = __builtin_amdgcn_alignbyte(a1, a0, sh), hi = __builtin_amdgcn_alignbyte(a2, a1, sh);   // byte j of (hi:lo) = tb[loc + j]
  uint64_t k = 0;
  if (gs.cyclic) {
    k = ((uint64_t)__builtin_bswap32(lo) << 24) | (uint64_t)(__builtin_bswap32(hi) >> 8);     // 7 bytes, first byte on top
    if (gs.packed) return ((k & 0xFFFFFFFFFFull) << PK_KEY_LO) | ((uint64_t)(t.seg & 1u) << PK_SHIFT) | (uint64_t)(t.off + loc);  // bytes 2..6 (two-phase sort): pk_record
    k >>= 8 * (7 - gs.nsym);
    k |= (uint64_t)(t.seg & 1u) << (8 * gs.nsym);
  } else {
    const uint32_t sn = t.seg + 1 == sg.nseg ? sg.n_last : sg.stride;
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    for (int j = 0; j < gs.nsym; j++) k = (k << 9) | (t.off + loc + j < sn ? (uint32_t)((both >> (8 * j)) & 0xFFu) + 1u : 0u);
    k |= (uint64_t)(t.seg & 1u) << (9 * gs.nsym);
  }
  return k;
}

// lanes of the wave that carry the same 8-bit digit.  Per bit: m = the bit spread over a word (v_bfe_i32), one ballot, and
// the lanes whose bit differs from mine are ballot ^ m, folded into the running OR by one v_bitop3 per half (q | (m ^ bal) =
// table 0xde): four VALU instructions per bit (the select form took nine).
__device__ __forceinline__ uint64_t match_any8(uint32_t d) {
  uint32_t qlo = 0, qhi = 0;
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)d, b, 1);      // 0 or ~0
    const uint64_t bal = __ballot(m != 0);
    qlo = __builtin_amdgcn_bitop3_b32(m, qlo, (uint32_t)bal, 0xde);
    qhi = __builtin_amdgcn_bitop3_b32(m, qhi, (uint32_t)(bal >> 32), 0xde);
  }
  return ~(((uint64_t)qhi << 32) | qlo);
}

// One ranking step of a wave: the number of keys with this lane's digit that the wave has seen before this lane's key (earlier
// steps, then lower lanes of this step); wc = the wave's 256 running digit counts.
// (Measured and dropped: taking the peer mask out of LDS instead of eight ballots -- every lane ORs its lane bit into the
// digit's 64-bit word, reads it back, the first lane clears it: 15 VALU + 5 DS instructions instead of ~70 VALU, bit-exact,
// but same-address LDS atomics are done one lane after the other and text digits put a dozen lanes on one word:
// rs_scatter 345 vs 320 us, tile sorter 1.07 ms both ways.)
__device__ __forceinline__ uint32_t rank_step(uint32_t d, uint32_t* __restrict__ wc) {
  const uint64_t peers = match_any8(d);
  const uint32_t prior = wc[d];
  const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
  __builtin_amdgcn_wave_barrier();
  if (r == 0) wc[d] = prior + (uint32_t)__popcll(peers);
  __builtin_amdgcn_wave_barrier();
  return prior + r;
}

}  // namespace cjs
