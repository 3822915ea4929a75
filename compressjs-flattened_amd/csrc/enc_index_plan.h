// enc_index_plan.h -- host arithmetic of the compressor's block rows (enc_index.hip makes them): the rows of the blocks
// a call, a shard or an encoder step has packed become the entries of the stream's block index and the counts of its line table.
// Plain integers and vectors.  No HIP in here (tests/host/enc_index_check.cc compiles it with the host compiler).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "cjs_hip.h"

namespace cjs {

// What the compressor knows of one block when it packs it: the bits it takes in the stream (its 48-bit magic and its CRC included),
// its CRC, the input bytes it holds and how many of them are 0x0A.
struct EncRow { uint32_t bits, crc, size, newlines; };
static_assert(sizeof(EncRow) == 16, "a row is four words");

constexpr uint64_t ENC_FIRST_BIT = 32;      // the first block of a stream stands behind 'BZh<level>'

// The entries and counts of `count` blocks that stand one behind the other from stream bit start_bit on, appended to entries and
// newlines (which stay parallel).  Returns the bit behind the last of them: the start_bit of the rows that follow.
inline uint64_t enc_rows_append(std::vector<cjs_bz_index_entry>& entries, std::vector<uint32_t>& newlines, const EncRow* rows, size_t count,
                                uint64_t start_bit, int level) {
  uint64_t bit = start_bit;
  for (size_t k = 0; k < count; k++) {
    cjs_bz_index_entry e;
    e.bitpos = bit; e.end_bit = bit + rows[k].bits;
    e.size = rows[k].size; e.crc = rows[k].crc; e.level = (uint32_t)level; e.reserved = 0;
    entries.push_back(e);
    newlines.push_back(rows[k].newlines);
    bit = e.end_bit;
  }
  return bit;
}

// the bytes of the stream whose last block ends at end_bit (no block: ENC_FIRST_BIT): the end-of-stream magic and the stream CRC
// stand behind it, the last byte is padded
inline uint64_t enc_stream_bytes(uint64_t end_bit) { return (end_bit + 80 + 7) / 8; }

}  // namespace cjs
