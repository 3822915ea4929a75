// rle1_rules.h — the arithmetic of stage 0 (RLE1 and its block boundaries), each rule once.  No HIP: plain constexpr functions
// that the kernels of rle1.hip, rle1_bytes.hip and rle1_batch.hip and the host compiler read alike
// (tests/host/rle1_rules_check.cc checks them against a byte-serial model of bzip2's block reader).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cjs {

// ---- the chunk rule.  A run of equal bytes is cut into chunks of at most 255; dp = offset of a byte in its chunk.  The first
// four bytes of a chunk are literals, the fourth brings the chunk's count byte with it, bytes 4..254 go into that count.
constexpr uint32_t chunk_emit(uint32_t dp) { return dp < 3 ? 1u : dp == 3 ? 2u : 0u; }     // output bytes of the byte at dp
constexpr uint32_t chunk_next(uint32_t dp) { return dp == 254 ? 0u : dp + 1u; }            // dp of the next byte of the run

// ---- one run chunked afresh from its first byte (the run that a block starts in)
// output bytes after m bytes of the run: 5 per whole chunk, then literals, then the count byte
constexpr uint64_t emitted_fresh(uint64_t m) { return 5 * (m / 255) + (m % 255 < 4 ? m % 255 : 5u); }
// output offset of byte d of the run, for d % 255 < 4 (the bytes behind go into the count byte at offset 5 * (d / 255) + 4)
constexpr uint64_t fresh_offset(uint64_t d) { return 5 * (d / 255) + (d % 255 < 4 ? d % 255 : 4u); }
// input bytes of the run after which a block of cap >= 1 output bytes is full: the smallest m with emitted_fresh(m) >= cap.
// A chunk's fifth output byte, the count, comes together with its fourth literal, so a multiple of five is reached at the
// fourth byte of the LAST chunk, not at that chunk's end: rem == 0 counts one whole chunk less.
constexpr uint64_t run_fill_input(uint32_t cap) {
  const uint32_t q = cap / 5, rem = cap % 5;
  return rem == 0 ? (uint64_t)255 * (q - 1) + 4 : (uint64_t)255 * q + rem;
}

// ---- tiles: the boundary pass works on 4 KiB tiles of the input
constexpr uint32_t RT = 4096;
constexpr uint32_t tiles_for(uint64_t n) { return (uint32_t)((n + RT - 1) / RT); }
// multi-GPU jobs: every rank makes the tile tables of this many consecutive tiles (a multiple of 4) and the ranks exchange them
constexpr uint32_t tiles_per_rank(uint64_t n, uint32_t world) { return ((tiles_for(n) + world - 1) / (world ? world : 1) + 3u) & ~3u; }
// One rank's share of the tile tables as it is exchanged, tpr tiles: lb u64[tpr] | fb u64[tpr] | gt u64[tpr] | subpre u16[tpr][16] |
// dmod u8[tpr][16].  Byte offsets of the sections and the size of the share; subpre and dmod are read 16 bytes at a time.
struct TileShare { size_t lb, fb, gt, subpre, dmod, bytes; };
constexpr TileShare tile_share(uint32_t tpr) { return {0, (size_t)8 * tpr, (size_t)16 * tpr, (size_t)24 * tpr, (size_t)56 * tpr, (size_t)72 * tpr}; }

// blocks of a stream of max_in bytes: a block takes at least 4/5 of its capacity in input bytes (four literals and a zero count)
constexpr size_t max_blocks_for(size_t max_in, uint32_t cap) { return max_in / ((size_t)cap * 4 / 5) + 2; }

}  // namespace cjs
