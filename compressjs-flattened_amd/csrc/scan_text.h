// scan_text.h -- the text of a tile in LDS, as the literal search (search.hip) and the regex search (regex.hip) both stage it: the
// tile's start positions and the halo behind them, loaded as aligned 16-byte vectors bounded to the segment, folded under NOCASE,
// the prefix bytes from the call's carry buffer.  Segments, carry and tiling are search_plan's (scan_plan.h).
#pragma once
#include "range_engine.h"

namespace cjs {

constexpr uint32_t SR_TILE = 16384;                                        // start positions of a tile (a power of two >= 1024)
constexpr uint32_t SR_ROWS = SR_TILE / 64;                                 // a row = the 64 positions a wave tests at once
constexpr uint32_t SR_MAXP = CJS_SEARCH_MAX_PATTERNS, SR_MAXL = CJS_SEARCH_MAX_PATTERN_BYTES;
constexpr uint32_t SR_TEXT = (15 + SR_TILE + SR_MAXL - 1 + 15) / 16 * 16 + 16;      // staged bytes at any alignment, + the word behind the last
static_assert(SR_ROWS == 256 && SR_MAXP == 64, "one row per thread of the block scan, one mask bit per pattern");

struct SrSeg : SearchSeg {};      // (scan_plan.h; the kernels' own name for it: the host hands them an array of SearchSeg)
struct SrTile { uint64_t off0, left; uint32_t npos, sh, npat; };      // decoded offset of and bytes from position 0; positions; its LDS byte

// 'A'..'Z' -> 'a'..'z' in the four bytes of w
__device__ __forceinline__ uint32_t sr_fold4(uint32_t w) {
  const uint32_t h = w & 0x7F7F7F7Fu;
  const uint32_t m = (h + 0x3F3F3F3Fu) & ~(h + 0x25252525u) & ~w & 0x80808080u;      // bit 7: 0x41 <= byte <= 0x5A
  return w | (m >> 2);
}

// Tile blockIdx.x: its segment and the tile's bytes (+ the halo of maxlen - 1) into text[SR_TEXT / 4].  Byte i of the tile is at
// LDS byte sh + i, congruent mod 16 to its device address, so the loads are aligned vectors bounded to the segment (rg_ld16).
// Ends behind a barrier: what the caller wrote to LDS in front of the call is visible too.  npat is the caller's to set.
__device__ __forceinline__ SrTile sr_stage_text(uint32_t* text, const SrSeg* __restrict__ segs, uint32_t nseg, uint32_t maxlen,
                                                const uint8_t* __restrict__ carry, uint32_t fold) {
  const uint64_t t = blockIdx.x;
  const SrSeg g = rg_seg_of(segs, nseg, t);
  const uint64_t p0 = (t - g.tile0) * SR_TILE, n = g.pre + g.len;
  SrTile T;
  T.npos = (uint32_t)min((uint64_t)SR_TILE, g.npos - p0);
  T.left = n - p0; T.off0 = g.off + p0; T.npat = 0;
  const uint32_t nbytes = (uint32_t)min(T.left, (uint64_t)(T.npos + maxlen - 1));
  const uint64_t a0 = g.src + p0 - g.pre;                                  // address of the tile's byte 0 (in front of src: the prefix)
  T.sh = (uint32_t)(a0 & 15u);
  const uint64_t s_lo = g.src + (p0 > g.pre ? p0 - g.pre : 0), s_hi = p0 + nbytes > g.pre ? g.src + min(g.len, p0 + nbytes - g.pre) : g.src;
  if (s_hi > s_lo) {
    const uint32_t nvec = (T.sh + nbytes + 15) / 16;
    for (uint32_t v = threadIdx.x; v < nvec; v += 256) {
      uint4 x = rg_ld16((a0 & ~15ull) + 16ull * v, s_lo, s_hi);
      if (fold) { x.x = sr_fold4(x.x); x.y = sr_fold4(x.y); x.z = sr_fold4(x.z); x.w = sr_fold4(x.w); }
      reinterpret_cast<uint4*>(text)[v] = x;
    }
  }
  __syncthreads();
  if (p0 < g.pre) {                                                          // the prefix: a few bytes of the carry buffer
    const uint32_t np = (uint32_t)min((uint64_t)nbytes, g.pre - p0);
    for (uint32_t j = threadIdx.x; j < np; j += 256) {
      uint8_t c = carry[p0 + j];
      if (fold && c >= 'A' && c <= 'Z') c += 32;
      reinterpret_cast<uint8_t*>(text)[T.sh + j] = c;
    }
  }
  __syncthreads();
  return T;
}

}  // namespace cjs
