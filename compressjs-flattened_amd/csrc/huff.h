// huff.h — Huffman table construction + bit packing stage buffers and entry points.
#pragma once
#include "cjs_internal.h"
#include "mtf.h"
#include "huff_rules.h"

namespace cjs {

struct HuffBufs {
  uint8_t* sel;       // [nb][sel_stride] table index per group of 50 symbols
  uint8_t* selj;      // [nb][sel_stride] MTF position of each selector (unary-coded in the stream)
  uint16_t* bcost;    // [nb][sel_stride] cost of each group under its selected table
  uint8_t* lens;      // [nb][6][258]
  uint32_t* codes;    // [nb][6][258] canonical codes
  uint32_t* ngroups;  // [nb]
  uint32_t* bitlen;   // [nb] bits of the block incl. its 48-bit magic and CRC
  uint64_t* bitoff;   // [nb+1] absolute bit offset of each block in the output
  uint32_t* databits; // [nb] bits of the block's symbol data (the last part of the block)
  uint32_t* tileoff;  // [nb][tile_stride] bit offset of every 80-group (4000-symbol) tile inside the symbol data
  uint8_t* wl;        // [nb][6][264] code lengths between the kernels of the split refinement
  uint32_t* wfreq;    // [nb][6][260] symbol counts per table, same
  size_t sel_stride, tile_stride;
};

struct HuffWork {
  size_t max_blocks = 0;
  uint32_t max_stride = 0;
  HuffBufs b{};
  uint64_t* scalars = nullptr;   // [0] total bits, [1] (u32) stream crc, [2] output too small
  static size_t sel_stride_for(uint32_t stride) { return cjs::sel_stride_for(stride); }
  static size_t bytes_needed(size_t max_blocks, uint32_t stride);
  int carve(Arena& a, size_t max_blocks, uint32_t stride);
  // the table-construction buffers seen from block `first` on (`count` blocks); bitoff / scalars belong to the packing of a whole call
  HuffWork view(size_t first, size_t count) const {
    HuffWork v = *this;
    v.max_blocks = count;
    v.b.sel += first * b.sel_stride; v.b.selj += first * b.sel_stride; v.b.bcost += first * b.sel_stride;
    v.b.lens += first * lens_row_bytes(); v.b.codes += first * codes_row_elems();
    v.b.ngroups += first; v.b.bitlen += first; v.b.databits += first; v.b.tileoff += first * b.tile_stride;
    v.b.wl += first * wl_row_bytes(); v.b.wfreq += first * wfreq_row_elems();
    return v;
  }
};

// which implementation builds the tables: HUFF_AUTO = by the shape of the call (what every production caller uses), or forced
// (the stage-level tests run both on the same blocks)
enum HuffPath { HUFF_AUTO = 0, HUFF_PER_BLOCK = 1, HUFF_CHAIN = 2 };
int huff_tables_run(hipStream_t s, HuffWork& w, uint32_t nb, const SymRows& r, int path = HUFF_AUTO);
// a rank of a multi-GPU job: the stream CRC folded over ALL ranks' blocks (the trailer writer needs it), and whether the next
// rank's blocks follow this fragment (pack_frame then completes the fragment's last word with the leading bits of the block magic)
struct PackShard { uint32_t stream_crc; int follow_magic; };
// What a pack run is told besides the symbol rows: blocks [first, first + count) of a stream of nb_total, from absolute bit
// start_bit of out32 on (the part the stream occupies is zeroed by the run, the bits in front of start_bit included).
struct PackJob {
  uint32_t nb_total, first, count;
  uint64_t start_bit;
  int level;
  bool header, trailer;              // 'BZh<level>' in front / end-of-stream magic and stream CRC behind
  const uint32_t *block_crc, *pidx;  // per block: block_crc indexed from block 0 of the stream, pidx from `first`
  uint32_t* out32;
  size_t out_cap_bytes;
  const PackShard* shard = nullptr;
};
int huff_pack_run(hipStream_t s, HuffWork& w, const SymRows& r, const PackJob& j);    // scalars[2] = 1 and nothing written if the stream does not fit

// Batches of independent streams (cjs_bzip2_compress_batch*), one per block: framed = header, block j, trailer; else block j's
// bare bit string from bit 0.  Item j lands at byte d_soff[j] (4-byte aligned, from `base` on, in block order); d_slen[j] = its
// length in bytes, w.scalars[0] = bytes of all of them (aligned).  The pack run writes them into j.out32, whose range
// [base, base + scalars[0]) the caller has zeroed; of the job it reads count, level, header (= framed), block_crc, pidx, out32.
int huff_batch_offsets_run(hipStream_t s, HuffWork& w, uint32_t nb, uint64_t base, int framed, uint64_t* d_soff, uint32_t* d_slen);
int huff_batch_pack_run(hipStream_t s, HuffWork& w, const SymRows& r, const PackJob& j, const uint64_t* d_soff);

// end-of-stream magic and stream CRC (48 + 32 bits) OR-ed into the big-endian words of out32 from stream bit `bit` on; returns
// the bit behind them.  One lane per stream (pack_frame, huff_batch_frame, batch_asm_frame).
__device__ __forceinline__ uint64_t put_trailer_words(uint32_t* out32, uint64_t bit, uint32_t crc) {
  const uint64_t vals[2] = {MAGIC_END, (uint64_t)crc};
  const uint32_t nbs[2] = {48, 32};
  for (int q = 0; q < 2; q++) {
    split_bits(bit, vals[q], nbs[q], [&](uint64_t w, uint32_t piece) { atomicOr(&out32[w], __builtin_bswap32(piece)); });
    bit += nbs[q];
  }
  return bit;
}

}  // namespace cjs
