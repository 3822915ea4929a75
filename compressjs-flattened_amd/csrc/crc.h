// crc.h — bzip2 CRC-32 of byte ranges on the device (crc.hip): the compressor's block CRCs over its input, the decoder's over
// its output.  A range is an RleBlock of which only s and e are read.
#pragma once
#include "crc32_bz.h"
#include "rle1.h"

namespace cjs {

// CRC-32 (bzip2 form) of byte ranges [d_blocks[k].s, d_blocks[k].e) of d_data, first <= k < min(first + count, *d_nblocks), to
// d_crc_out[k]; d_seg_crc holds count * max_segs words, max_segs >= crc_segs_for(longest range)
int crc_ranges_at(hipStream_t s, const uint8_t* d_data, const RleBlock* d_blocks, const uint32_t* d_nblocks, uint32_t first, uint32_t count,
                  uint32_t max_segs, uint32_t* d_seg_crc, uint32_t* d_crc_out);
// the same from range 0
int crc_ranges(hipStream_t s, const uint8_t* d_data, const RleBlock* d_blocks, const uint32_t* d_nblocks, uint32_t count, uint32_t max_segs,
               uint32_t* d_seg_crc, uint32_t* d_crc_out);

}  // namespace cjs
