// bz_frame.h — host arithmetic of a .bz2 stream's frame: the stream CRC fold, the layout of the ranks' bit strings in the one
// stream, the bit-string stitcher and the trailer.  No HIP in here (tests/host/frame_check.cc compiles it with the host compiler).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace cjs {

// block magic (pi), end-of-stream magic (sqrt pi), 48 bits each; the stream's first word is BZH0_WORD + level
constexpr uint64_t MAGIC_BLOCK = 0x314159265359ull, MAGIC_END = 0x177245385090ull;
constexpr uint32_t BZH0_WORD = 0x425a6830u;      // 'B' 'Z' 'h' '0'

// stream CRC after one more block: c -> rol1(c) ^ crc (J/Bzip2_joined_.js:2237)
inline uint32_t crc_fold(uint32_t c, uint32_t crc) { return ((c << 1) | (c >> 31)) ^ crc; }
// ... after `blocks` more blocks whose CRCs folded from 0 give `fold`: c -> rol(c, blocks) ^ fold
inline uint32_t crc_fold_join(uint32_t c, uint64_t blocks, uint32_t fold) {
  const uint32_t rot = (uint32_t)(blocks & 31u);
  return (rot ? ((c << rot) | (c >> (32 - rot))) : c) ^ fold;
}

// global bit offset of rank `rank`'s first block, stream CRC (the ranks' folds chained), the rank that ends the stream (the last
// one with blocks) and the stream's bit length without the trailer.  Meta: cjs_shard_meta (bits, blocks, crc_fold are read).
// starts (optional): the bit offset of every rank's first block.
template <typename Meta>
inline void shard_layout(const Meta* metas, int world, int rank, uint64_t& start, uint64_t& total, uint32_t& scrc, int& writer, uint64_t* starts = nullptr) {
  start = 32; total = 32; scrc = 0; writer = 0;
  for (int r = 0; r < world; r++) {
    if (r < rank) start += metas[r].bits;
    if (starts) starts[r] = total;
    total += metas[r].bits;
    scrc = crc_fold_join(scrc, metas[r].blocks, metas[r].crc_fold);
    if (metas[r].blocks) writer = r;
  }
}

// dst bits [pos, pos + nbits) |= the first nbits bits of src (MSB first); src is readable 9 bytes past its last bit.  Bytes
// that lie wholly inside the range are STORED (8 at a time, one 64-bit funnel shift), the partial bytes at the two ends OR-ed
// (the neighbours' bits live there): ranges of different shards may be merged by different threads when `edges` tells them
// apart -- 0: interior only (parallel part), 1: the two ends only (serial part).
inline void funnel_merge(uint8_t* dst, uint64_t pos, const uint8_t* src, uint64_t nbits, int edges) {
  auto src_bits = [&](uint64_t off, unsigned k) -> uint32_t {             // k <= 8 bits of src from bit `off`
    uint32_t v = 0;
    for (unsigned i = 0; i < k; i++) { const uint64_t b = off + i; v = (v << 1) | ((src[b >> 3] >> (7 - (b & 7))) & 1u); }
    return v;
  };
  const uint64_t end = pos + nbits;
  const uint64_t j0 = (pos + 7) >> 3, j1 = end >> 3;                      // whole bytes of dst inside the range: [j0, j1)
  if (edges) {
    if (j0 > j1) { const unsigned k = (unsigned)nbits; dst[pos >> 3] |= (uint8_t)(src_bits(0, k) << (8 - (pos & 7) - k)); return; }   // inside one byte
    if (pos & 7) { const unsigned k = 8 - (unsigned)(pos & 7); dst[pos >> 3] |= (uint8_t)src_bits(0, k); }
    if (end & 7) { const unsigned k = (unsigned)(end & 7); dst[end >> 3] |= (uint8_t)(src_bits(nbits - k, k) << (8 - k)); }
    return;
  }
  if (j0 >= j1) return;
  const uint64_t o = 8 * j0 - pos;                                        // src bit of dst byte j0 (< 8)
  const unsigned r = (unsigned)(o & 7);
  const uint8_t* q = src + (o >> 3);
  uint64_t j = j0;
  for (; j + 8 <= j1; j += 8, q += 8) {
    uint64_t hi; memcpy(&hi, q, 8); hi = __builtin_bswap64(hi);
    const uint64_t v = r ? (hi << r) | ((uint64_t)q[8] >> (8 - r)) : hi;
    const uint64_t be = __builtin_bswap64(v);
    memcpy(dst + j, &be, 8);
  }
  for (; j < j1; j++, q++) dst[j] = r ? (uint8_t)((q[0] << r) | (q[1] >> (8 - r))) : q[0];
}

// end-of-stream magic and stream CRC (48 + 32 bits) OR-ed into `bytes` (zero there) from bit `bit` on
inline void put_trailer(uint8_t* bytes, uint64_t bit, uint32_t crc) {
  const uint64_t vals[2] = {MAGIC_END, crc}; const int nbs[2] = {48, 32};
  for (int q = 0; q < 2; q++) for (int i = nbs[q] - 1; i >= 0; i--, bit++) if ((vals[q] >> i) & 1) bytes[bit >> 3] |= (uint8_t)(0x80 >> (bit & 7));
}

}  // namespace cjs
