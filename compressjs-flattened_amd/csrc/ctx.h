// ctx.h — the per-GPU context behind the opaque cjs_ctx of the C ABI (pipeline.hip: single streams and the shard phases;
// enc_host.hip: the host-buffer driver; enc_stream.hip: the streaming encoder; batch.hip: batches).
#pragma once
#include "cjs_internal.h"
#include "bz_frame.h"
#include "rle1.h"
#include "mtf.h"
#include "huff.h"
#include "enc_index.h"

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
  cjs::Owner<cjs::EncRowsWork*, cjs::EncRowsDelete> enc_rows;   // the block rows of the indexed calls (enc_index.hip), made by the first one
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
// All of these: pipeline.hip.
// blocks [f, f + cnt) of the stream whose boundaries c->rle holds (rle1_run: nb blocks, the last of last_len bytes)
// through RLE1 bytes / CRCs, suffix sort, MTF / RLE2 and the Huffman tables; the caller packs (pack_enqueue)
int blocks_through_tables(cjs_ctx* c, const uint8_t* d_in, size_t n, uint32_t nb, uint32_t last_len, uint32_t f, uint32_t cnt, cjs_stats* st, bool stage_times);
// The packing of those blocks on the context's stream, in two halves (a caller may enqueue more between them):
// pack_enqueue: huff_pack_run over the context's symbol rows, then the copy of the run's scalars to the host;
// pack_finish: waits for the stream; CJS_E_OUTPUT_TOO_SMALL if the stream did not fit, else *end_bit = the bit behind what was written
int pack_enqueue(cjs_ctx* c, const PackJob& j);
int pack_finish(cjs_ctx* c, uint64_t* end_bit);
// The body of cjs_bzip2_compress_device (first = 0, count = -1, framed) and cjs_bzip2_compress_device_range (bare bit strings).
// want (may be null: the plain calls): the rows of the packed blocks are appended to it (enc_index.h), brought down in front of
// pack_finish's wait.
int compress_core(cjs_ctx* c, const uint8_t* d_in, size_t n, int level, long first, long count, bool framed, uint8_t* d_out, size_t out_cap,
                  uint64_t* out_bits, uint32_t* block_crcs, long crc_cap, long* total_blocks, cjs_stats* st, EncRowsWant* want = nullptr);
// rc; after an error (rc != 0) the context's three streams have drained first: an early return may leave kernels in flight (block
// CRCs on the side stream, MTF / Huffman tables of earlier pieces on the tail stream) against a context the caller reuses
int drain_on_error(cjs_ctx* c, int rc);
// The bodies of cjs_bzip2_shard_blocks (without drain_on_error: the caller's) and of cjs_bzip2_shard_pack behind shard_layout,
// which the worker threads of the host-buffer driver (enc_host.hip) run on byte ranges that are streams of their own.
int shard_blocks_impl(cjs_ctx* c, const uint8_t* d_in, size_t n, int level, int rank, int world, const void* d_shares, cjs_shard_meta* meta, cjs_stats* st,
                      EncRowsWant* want = nullptr);      // want: as for compress_core, the rows of the rank's blocks
int shard_pack_core(cjs_ctx* c, int level, bool header, bool trailer, uint64_t start, uint64_t bits, uint32_t scrc, uint8_t* d_out, size_t out_cap,
                    size_t* frag_off, size_t* frag_len, uint64_t* stream_off);
}  // namespace cjs
