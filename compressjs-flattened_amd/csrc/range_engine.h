// range_engine.h -- the pass engine of the indexed entry points (range.hip defines it): the blocks an index names go through phases
// A, B and C in bounded passes, each judged against its entry, and every decoded inverse-BWT batch is handed to a consumer while it
// stands expanded in device scratch.  Four consumers: the slice gather of the range reads (range.hip), the pattern scan
// (search.hip), the newline count, select and rank of the line table (lines.hip) and the compare (compare.hip).
#pragma once
#include "dec_engine.h"
#include "bz_index.h"
#include <functional>
#include <vector>

namespace cjs {

enum { RG_GOOD = 0, RG_MISMATCH = 1, RG_BAD_CRC = 2 };      // a touched block against its index entry

// The aligned 16 bytes at address p of a source that is bytes [lo, hi): a vector load when they all belong to it; at the two ends
// of a source the bytes that do, one by one, zeros for the others (nothing outside the source is read).
__device__ __forceinline__ uint4 rg_ld16(uint64_t p, uint64_t lo, uint64_t hi) {
  if (p >= lo && p + 16 <= hi) return *reinterpret_cast<const uint4*>(p);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 16; i++) if (p + i >= lo && p + i < hi) w[i >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(p + i) << (8 * (i & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

struct RangeStats { uint64_t h2d = 0, d2h = 0, up = 0; uint32_t passes = 0, a_batches = 0, b_batches = 0; size_t slices = 0; };

// One decoded batch of a pass: chain blocks [g0, g1), chain block k being index block blk[k], out_len bytes at byte J.out_off[k]
// of d_exp (a block of the wrong size or with a bad CRC takes its room there all the same), its verdict already in the engine's
// verdict array.  q: scratch for the batch's duration; s: the pass's stream.
struct RangeBatch {
  const DecJob& J; DecShare& S; const std::vector<uint32_t>& blk;
  size_t g0, g1; uint8_t* d_exp; ShareScratch& q; hipStream_t s;
};
// returns with the stream drained
using RangeConsumer = std::function<int(const RangeBatch&)>;

// in: the stream on the host, or nullptr with d_src: the stream on device `dev`.  touched: the blocks to decode, ascending.
// verdict / crc_got: per block of the index (RG_*; the computed CRC of an RG_BAD_CRC block), written for the touched blocks.
int range_engine(const uint8_t* in, const uint8_t* d_src, const cjs_bz_index* ix, const std::vector<uint32_t>& touched,
                 std::vector<uint8_t>& verdict, std::vector<uint32_t>& crc_got, int dev, RangeStats& st, const RangeConsumer& consume);
// The range reads on the engine, the result in device memory: range k ([off[k], off[k] + len[k]) clipped to total_bytes) at d_out +
// the sum of the clipped lengths in front of it, from the stream on the host (`in`) or on device `dev` (d_src).  The region of a
// range that touches a bad block holds unspecified bytes; the verdicts say which blocks were bad.
int range_read_to_device(const uint8_t* in, const uint8_t* d_src, const cjs_bz_index* ix, const uint64_t* off, const uint64_t* len, size_t count,
                         uint8_t* d_out, std::vector<uint8_t>& verdict, std::vector<uint32_t>& crc_got, int dev, RangeStats& st);
// the detail text of bad block `bad`: one of read_ranges' two
void range_bad_detail(const cjs_bz_index* ix, size_t bad, const std::vector<uint8_t>& verdict, const std::vector<uint32_t>& crc_got);
// the block that holds decoded offset o < total_bytes (of non-zero size)
inline size_t range_block_of(const cjs_bz_index* ix, uint64_t o) { return (size_t)(std::upper_bound(ix->off.begin(), ix->off.end(), o) - ix->off.begin()) - 1; }

}  // namespace cjs
