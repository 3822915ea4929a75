// rle1.h — stage 0 (RLE1 + block boundaries + CRC) workspace and entry points: rle1.hip (boundaries), rle1_bytes.hip (bytes, CRCs),
// rle1_batch.hip (batches of inputs).  The rules of the arithmetic: rle1_rules.h; the CRC of byte ranges: crc.h.
#pragma once
#include "cjs_internal.h"
#include "crc32_bz.h"
#include "rle1_rules.h"

namespace cjs {

struct RleBlock {
  uint64_t s, e;       // input range consumed by the block
  uint64_t r_end;      // end of the run that contains s (block-fresh chunking applies to [s, r_end))
  uint64_t Gr;         // global emitted-byte prefix at r_end
  uint32_t len;        // RLE1 output length (== cap for every block but possibly the last)
  uint32_t base;       // bytes emitted by the first (re-chunked) run
};

struct Rle1Work {
  size_t max_in = 0;
  uint32_t cap = 0, max_blocks = 0, max_segs = 0, range_blocks = 0;
  Pinned<uint32_t> h_n;          // host scalar
  uint64_t *fb = nullptr, *lb = nullptr, *gt = nullptr;
  unsigned long long* agg = nullptr;     // chunk aggregates of the three-phase tile scans
  uint16_t* subpre = nullptr;    // [tiles][16] emitted bytes of the tile before each 256-byte subtile
  uint8_t* dmod = nullptr;       // [tiles][16] chunk phase of each subtile's first byte
  RleBlock* blocks = nullptr;
  uint32_t *block_len = nullptr, *block_crc = nullptr, *nblocks = nullptr, *seg_crc = nullptr;
  static size_t max_blocks_for(size_t max_in, uint32_t cap) { return cjs::max_blocks_for(max_in, cap); }
  static size_t max_segs_for(uint32_t cap) { return crc_segs_for((size_t)cap * 51); }     // a block takes at most 51 input bytes per output byte (255 for 5)
  // multi-GPU jobs: every rank makes the tile tables of `tiles_per_rank` consecutive 4 KiB tiles and the ranks exchange them
  // (the layout of one share: tile_share() of rle1_rules.h)
  static uint32_t tiles_for(uint64_t n) { return cjs::tiles_for(n); }
  static uint32_t tiles_per_rank(uint64_t n, uint32_t world) { return cjs::tiles_per_rank(n, world); }
  static size_t share_bytes(uint32_t tpr) { return tile_share(tpr).bytes; }
  // range_blocks = max number of blocks materialised / CRC'd per call (0 = all blocks of the stream)
  static size_t bytes_needed(size_t max_in, uint32_t cap, size_t range_blocks = 0);
  int carve(Arena& a, size_t max_in, uint32_t cap, size_t range_blocks = 0);
};

int rle1_run(hipStream_t s, Rle1Work& w, const uint8_t* d_in, uint64_t N, uint32_t* nblocks_host, uint32_t* last_len_host = nullptr);
// the two halves of rle1_run for jobs that shard the tile passes over ranks (see rle1.hip)
int rle1_tiles(hipStream_t s, Rle1Work& w, const uint8_t* d_in, uint64_t N, uint32_t t0, uint32_t t1, uint8_t* share, uint32_t tpr);
int rle1_tables_from_shares(hipStream_t s, Rle1Work& w, uint64_t N, const uint8_t* d_recv, uint32_t tpr);
int rle1_walk_run(hipStream_t s, Rle1Work& w, const uint8_t* d_in, uint64_t N, uint32_t* nblocks_host, uint32_t* last_len_host = nullptr);
// Batches of independent inputs (input k = d_in[d_se[2k] .. d_se[2k+1]), d_se on the device):
//   rle1_batch_len: RLE1 length of every input, d_len2[k] = min(len, cap + 1) << 1 | (last byte absorbed into a run-length byte);
//   rle1_batch_walk: block boundaries of the inputs d_item[0..count) (RleBlock s / e relative to the input, len), at most
//     d_tbase[j+1] - d_tbase[j] of them from d_blocks + d_tbase[j], their number to d_nblk[j];
//   rle1_batch_materialize: RLE1 bytes of blocks d_blk[0..nb) (s / e relative to d_in), block j at d_blocks + j*stride.
int rle1_batch_len(hipStream_t s, const uint8_t* d_in, const uint64_t* d_se, uint32_t count, uint32_t cap, uint64_t* d_len2);
int rle1_batch_walk(hipStream_t s, const uint8_t* d_in, const uint64_t* d_se, const uint32_t* d_item, const uint32_t* d_tbase, uint32_t count,
                    uint32_t cap, RleBlock* d_blocks, uint32_t* d_nblk);
int rle1_batch_materialize(hipStream_t s, const uint8_t* d_in, const RleBlock* d_blk, uint32_t nb, uint32_t stride, uint8_t* d_blocks);
int rle1_finish(hipStream_t s, Rle1Work& w, const uint8_t* d_in, uint64_t N, uint32_t first, uint32_t count, uint8_t* d_blocks,
                hipStream_t side = nullptr, hipEvent_t ev_fork = nullptr, hipEvent_t ev_join = nullptr);

}  // namespace cjs
