// ctx.h — the per-GPU context behind the opaque cjs_ctx of the C ABI (pipeline.hip: single streams; batch.hip: batches).
#pragma once
#include "cjs_internal.h"
#include "rle1.h"
#include "mtf.h"
#include "huff.h"

namespace cjs {
struct BatchWork;
void batch_destroy(BatchWork* b);                                // delete b (batch.hip, where BatchWork is complete)
struct BatchDelete { void operator()(BatchWork* b) const { batch_destroy(b); } };
}  // namespace cjs

// Members are destroyed in reverse order: the timer, events and streams first, the workspace last.  cjs_ctx_destroy makes the
// context's device current first.
struct cjs_ctx {
  int device = 0, level = 0;
  uint32_t cap = 0;
  size_t max_input = 0, max_blocks = 0, range_blocks = 0;
  cjs::Arena arena;
  cjs::Rle1Work rle;
  cjs::BwtWork bwt;
  cjs::MtfWork mtf;
  cjs::HuffWork huff;
  uint8_t* d_blocks = nullptr;
  uint8_t* d_U = nullptr;
  uint32_t* d_pidx = nullptr;
  cjs::Owner<cjs::BatchWork*, cjs::BatchDelete> batch;   // cjs_ctx_create_batch: workspace of the batch path (batch.hip)
  cjs::Pinned<uint64_t> h_scalars;
  cjs::Stream stream;
  cjs::Stream side;                // block CRCs run here, beside the suffix sort
  cjs::Event ev_join, ev_fork;
  cjs::Stream tail;                // MTF / Huffman tables of a finished piece run here, beside the suffix sort of the next piece
  cjs::Event ev_tail, ev_piece[8];
  cjs::EventTimer timer;
  // phase state of a multi-GPU job (cjs_bzip2_shard_tiles -> _blocks -> _pack)
  uint32_t sh_nb = 0, sh_first = 0, sh_cnt = 0, sh_state = 0;
  bool stage_times = true;         // cjs_ctx_set_stage_times
};

namespace cjs {
// pipeline.hip: blocks [f, f + cnt) of the stream whose boundaries c->rle holds (rle1_run: nb blocks, the last of last_len bytes)
// through RLE1 bytes / CRCs, suffix sort, MTF / RLE2 and the Huffman tables; the caller packs (huff_pack_run)
int blocks_through_tables(cjs_ctx* c, const uint8_t* d_in, size_t n, uint32_t nb, uint32_t last_len, uint32_t f, uint32_t cnt, cjs_stats* st, bool stage_times);
}  // namespace cjs
