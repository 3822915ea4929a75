// pipeline.hip — per-GPU context (workspace + stream) and the bzip2 compress pipeline on it:
//   RLE1/CRC/boundaries -> batched cyclic BWT -> MTF/RLE2 -> Huffman tables -> bit packing,
// as one stream (cjs_bzip2_compress_device[_range]) and as the three phases of a one-process-per-GPU job (cjs_bzip2_shard_*).
// Mirrors the block loop of Bzip2.compressFile (J/Bzip2_joined_.js:2199-2249) for all blocks at once.
// The host-buffer driver on top of it: enc_host.hip; the stage-level test entry points: stages.hip.
#include "ctx.h"
#include "enc_pieces.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>

using namespace cjs;


extern "C" int cjs_ctx_create(cjs_ctx** out, int device, size_t max_input, int level) {
  return cjs_ctx_create_sharded(out, device, max_input, 0, level);
}

extern "C" int cjs_ctx_create_sharded(cjs_ctx** out, int device, size_t max_input, long max_range_blocks, int level) {
  CJS_GUARD_BEGIN
  if (!out) return CJS_E_INVALID_ARG;
  *out = nullptr;
  if (level < 1 || level > 9) return CJS_E_BAD_LEVEL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CJS_E_NO_DEVICE;
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return CJS_E_NO_DEVICE; }
  if (device >= ndev) return CJS_E_INVALID_ARG;
  CJS_HIP_TRY(hipSetDevice(device));
  std::unique_ptr<cjs_ctx> c(new (std::nothrow) cjs_ctx());
  if (!c) return CJS_E_OUT_OF_MEMORY;
  c->device = device; c->level = level; c->cap = (uint32_t)level * 100000u - 19u;
  if (max_input == 0) max_input = 1;
  c->max_input = max_input;
  c->max_blocks = Rle1Work::max_blocks_for(max_input, c->cap);
  c->range_blocks = (max_range_blocks > 0 && (size_t)max_range_blocks < c->max_blocks) ? (size_t)max_range_blocks : c->max_blocks;
  const size_t rb = c->range_blocks;
  const size_t elems = rb * c->cap;
  size_t bytes = Rle1Work::bytes_needed(max_input, c->cap, rb) + BwtWork::bytes_needed(elems) +
                 MtfWork::bytes_needed(rb, c->cap) + HuffWork::bytes_needed(rb, c->cap) +
                 2 * (elems + 512) + 4 * rb + 65536;
  CJS_TRY(c->arena.init(bytes));
  CJS_TRY(c->rle.carve(c->arena, max_input, c->cap, rb));
  CJS_TRY(c->bwt.carve(c->arena, elems));
  CJS_TRY(c->mtf.carve(c->arena, rb, c->cap));
  CJS_TRY(c->huff.carve(c->arena, rb, c->cap));
  c->d_blocks = c->arena.take<uint8_t>(elems);
  c->d_U = c->arena.take<uint8_t>(elems);
  c->d_pidx = c->arena.take<uint32_t>(rb);
  if (!c->d_pidx) return CJS_E_OUT_OF_MEMORY;
  CJS_HIP_TRY(hipStreamCreate(c->stream.put()));
  CJS_HIP_TRY(hipStreamCreateWithFlags(c->side.put(), hipStreamNonBlocking));
  CJS_HIP_TRY(hipStreamCreateWithFlags(c->tail.put(), hipStreamNonBlocking));
  for (auto& e : c->ev_piece) CJS_HIP_TRY(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
  CJS_HIP_TRY(hipEventCreateWithFlags(c->ev_tail.put(), hipEventDisableTiming));
  CJS_HIP_TRY(hipEventCreateWithFlags(c->ev_fork.put(), hipEventDisableTiming));
  CJS_HIP_TRY(hipEventCreateWithFlags(c->ev_join.put(), hipEventDisableTiming));
  CJS_HIP_TRY(hipHostMalloc((void**)c->h_scalars.put(), 256));
  CJS_TRY(c->timer.init(c->stream));
  *out = c.release();
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" void cjs_ctx_set_stage_times(cjs_ctx* c, int on) { if (c) c->stage_times = on != 0; }

extern "C" void cjs_ctx_destroy(cjs_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  delete c;
}

int cjs::drain_on_error(cjs_ctx* c, int rc) {
  if (rc && c)
    for (hipStream_t s : {c->side.p, c->tail.p, c->stream.p}) if (s) (void)hipStreamSynchronize(s);
  return rc;
}

namespace {
// The timers of a call that fills a cjs_stats (st may be null: no timers): the whole call on an event pair of its own, and, with
// per-stage times on, the context's stage timer started for the first stage.
struct CallTimes {
  cjs_ctx* c = nullptr;
  cjs_stats* st = nullptr;
  bool stages = false;
  EventTimer whole;
  int begin(cjs_ctx* ctx, cjs_stats* stats) {
    c = ctx; st = stats; stages = st && c->stage_times;
    if (st) { memset(st, 0, sizeof *st); CJS_TRY(whole.init(c->stream)); whole.start(); }
    if (stages) c->timer.start();
    return 0;
  }
  void end(uint32_t cnt, size_t n, uint64_t bits) {        // the stream has drained
    if (!st) return;
    if (!stages && cnt) c->bwt.lt.resolve(st);
    st->ms_total = whole.stop();
    st->blocks = cnt; st->bytes_in = n; st->bytes_out = (bits + 7) / 8;
  }
};

// bytes of blocks from which blocks_through_tables goes in pieces (read at every call: tests shrink it)
uint64_t enc_piece_bytes() {
  const char* v = getenv("CJS_ENC_PIECE_BYTES");
  const unsigned long long x = v ? strtoull(v, nullptr, 10) : 0;
  return x ? (uint64_t)x : ENC_PIECE_BYTES;
}
}  // namespace

// blocks [f, f + cnt) of the stream whose boundaries the context's tables hold (nb blocks in all): RLE1 bytes + CRCs, suffix
// sort, MTF / RLE2, Huffman tables.  Everything but the bit packing; nothing here waits for the stream.  (Also the step of the
// streaming encoder, enc_stream.hip.)
int cjs::blocks_through_tables(cjs_ctx* c, const uint8_t* d_in, size_t n, uint32_t nb, uint32_t last_len, uint32_t f, uint32_t cnt, cjs_stats* st, bool stage_times) {
  hipStream_t s = c->stream;
  if (cnt > c->range_blocks) return CJS_E_INVALID_ARG;
  uint32_t n_last = c->cap;
  if (cnt && f + cnt == nb) n_last = last_len;        // (came to the host with the block count)
  // all per-block buffers below are indexed relative to `f`; only rle.block_len / block_crc are absolute
  CJS_TRY(rle1_finish(s, c->rle, d_in, n, f, cnt, c->d_blocks, c->side, c->ev_fork, c->ev_join));
  if (stage_times) { CJS_HIP_TRY(hipStreamSynchronize(s)); st->ms_rle1 = c->timer.stop(); }
  // The suffix sort keeps the memory system busy and the SIMDs idle; MTF / RLE2 and the Huffman tables are latency-bound chains
  // of small kernels that leave the memory system idle.  So the blocks go in `pieces` runs: while the sort of piece i + 1 runs on
  // the work stream, MTF and the tables of piece i run beside it on the tail stream (per-stage times: one piece, one stream).
  // Every piece pays the sort's ~90 launches again (each followed by ~6 us in which its write-back drains, and the tail rounds are
  // launch-bound whatever the piece holds): 100 MB in 2 / 3 / 4 pieces 12.5 / 13.2 / 14.2 ms against 11.7 in one; 2^30 bytes
  // (1,194 blocks) in 1 / 2 / 4 / 8 pieces 117.4 / 111.4 / 109.4 / 111.6 ms.  So: four pieces from 400 MB of blocks on.
  // (the rule: enc_pieces.h)
  const TablePieces tp = table_pieces(cnt, c->cap, enc_piece_bytes(), stage_times, c->tail.p != nullptr);
  const uint32_t runs = table_piece_count(cnt, tp);
  // One piece: its "tail" stream is the work stream itself, so no event orders the two and the sort's dominant-kernel events stay
  // where bwt_run left them.  The stage timers only ever run with one piece.
  const bool split = tp.pieces > 1;
  hipStream_t ts = split ? c->tail.p : s;
  LaunchTimes keep;                                        // the dominant-kernel events of all pieces are resolved together
  uint32_t rounds = 0;                                     // bwt_run reports the rounds of its own blocks: the call reports the most
  for (uint32_t i = 0; i < runs; i++) {
    uint32_t k0, kc;
    table_piece(cnt, tp, i, k0, kc);
    const bool has_last = k0 + kc == cnt;
    if (stage_times) c->timer.start();
    CJS_TRY(bwt_run(s, c->bwt, c->d_blocks + (size_t)k0 * c->cap, kc, c->cap, has_last ? n_last : c->cap, true, c->d_U + (size_t)k0 * c->cap, c->d_pidx + k0, st, stage_times));
    if (st) { rounds = std::max(rounds, st->bwt_rounds); st->bwt_rounds = rounds; }
    if (stage_times) { st->ms_bwt = c->timer.stop(); c->timer.start(); }
    if (split) {
      if (st) { c->bwt.lt.move_into(keep); }
      CJS_HIP_TRY(hipEventRecord(c->ev_piece[i], s));
      CJS_HIP_TRY(hipStreamWaitEvent(ts, c->ev_piece[i], 0));
    }
    MtfWork mv = c->mtf.view(k0, kc);
    HuffWork hv = c->huff.view(k0, kc);
    CJS_TRY(mtf_run(ts, mv, c->d_U + (size_t)k0 * c->cap, kc, c->rle.block_len + f + k0));
    if (stage_times) { CJS_HIP_TRY(hipStreamSynchronize(s)); st->ms_mtf = c->timer.stop(); c->timer.start(); }
    CJS_TRY(huff_tables_run(ts, hv, kc, mv.rows()));
    if (stage_times) { CJS_HIP_TRY(hipStreamSynchronize(s)); st->ms_huff = c->timer.stop(); }
  }
  if (split && cnt) {
    if (st) keep.move_into(c->bwt.lt);
    CJS_HIP_TRY(hipEventRecord(c->ev_tail, c->tail));
    CJS_HIP_TRY(hipStreamWaitEvent(s, c->ev_tail, 0));
  }
  if (cnt && env_debug()) fprintf(stderr, "[cjs pieces] blocks [%u, %u) of %u: %u pieces of up to %u blocks\n", f, f + cnt, nb, runs, tp.per);
  return 0;
}

int cjs::pack_enqueue(cjs_ctx* c, const PackJob& j) {
  // (the output size check is made on the device, by huff_offsets: no host round trip in front of the packing)
  CJS_TRY(huff_pack_run(c->stream, c->huff, c->mtf.rows(), j));
  CJS_HIP_TRY(hipMemcpyAsync(c->h_scalars, c->huff.scalars, 24, hipMemcpyDeviceToHost, c->stream));
  return 0;
}
int cjs::pack_finish(cjs_ctx* c, uint64_t* end_bit) {
  CJS_HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->h_scalars[2]) return CJS_E_OUTPUT_TOO_SMALL;
  *end_bit = c->h_scalars[0];
  return 0;
}

// Shared body: stage 0..tables for the whole stream, then pack blocks [first, first+count).
static int compress_core_impl(cjs_ctx* c, const uint8_t* d_in, size_t n, int level, long first, long count, bool framed,
                              uint8_t* d_out, size_t out_cap, uint64_t* out_bits, uint32_t* block_crcs, long crc_cap,
                              long* total_blocks, cjs_stats* st, EncRowsWant* want) {
  if (!c || level != c->level) return CJS_E_INVALID_ARG;
  if (n > c->max_input) return CJS_E_INVALID_ARG;
  if (((uintptr_t)d_out & 3) != 0) return CJS_E_INVALID_ARG;
  CJS_HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  c->sh_state = 0;
  CallTimes t;
  CJS_TRY(t.begin(c, st));
  uint32_t nb = 0, last_len = 0;
  CJS_TRY(rle1_run(s, c->rle, d_in, n, &nb, &last_len));
  if (total_blocks) *total_blocks = (long)nb;
  if (first < 0 || first > (long)nb) return CJS_E_INVALID_ARG;
  if (count < 0 || first + count > (long)nb) count = (long)nb - first;
  const uint32_t f = (uint32_t)first, cnt = (uint32_t)count;
  CJS_TRY(blocks_through_tables(c, d_in, n, nb, last_len, f, cnt, st, t.stages));
  if (t.stages) c->timer.start();
  if (cnt && n && c->side) CJS_HIP_TRY(hipStreamWaitEvent(s, c->ev_join, 0));      // block CRCs (side stream) before the headers are packed
  CJS_TRY(pack_enqueue(c, PackJob{nb, f, cnt, framed ? 32u : 0u, level, framed, framed, c->rle.block_crc, c->d_pidx, (uint32_t*)d_out, out_cap & ~(size_t)3}));
  if (block_crcs && nb) {
    if ((long)nb > crc_cap) return CJS_E_OUTPUT_TOO_SMALL;
    CJS_HIP_TRY(hipMemcpyAsync(block_crcs, c->rle.block_crc, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  }
  if (want) CJS_TRY(enc_rows_enqueue(c, d_in, n, f, cnt, want->lines));      // (behind the packing: the rows come down with its scalars)
  CJS_TRY(pack_finish(c, out_bits));
  if (want) enc_rows_collect(c, cnt, *want);
  if (t.stages) st->ms_pack = c->timer.stop();
  t.end(cnt, n, *out_bits);
  return 0;
}
int cjs::compress_core(cjs_ctx* c, const uint8_t* d_in, size_t n, int level, long first, long count, bool framed,
                       uint8_t* d_out, size_t out_cap, uint64_t* out_bits, uint32_t* block_crcs, long crc_cap,
                       long* total_blocks, cjs_stats* st, EncRowsWant* want) {
  CJS_GUARD_BEGIN
  return drain_on_error(c, compress_core_impl(c, d_in, n, level, first, count, framed, d_out, out_cap, out_bits, block_crcs, crc_cap, total_blocks, st, want));
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_compress_device(cjs_ctx* c, const uint8_t* d_in, size_t n, int level, uint8_t* d_out, size_t out_cap,
                                         size_t* out_n, cjs_stats* stats) {
  uint64_t bits = 0;
  CJS_TRY(compress_core(c, d_in, n, level, 0, -1, true, d_out, out_cap, &bits, nullptr, 0, nullptr, stats));
  *out_n = (size_t)((bits + 7) / 8);
  return 0;
}

extern "C" int cjs_bzip2_compress_device_indexed(cjs_ctx* c, const uint8_t* d_in, size_t n, int level, uint8_t* d_out, size_t out_cap,
                                                 size_t* out_n, cjs_bz_index** idx, cjs_bz_lines** lines, cjs_stats* stats) {
  if (idx) *idx = nullptr;
  if (lines) *lines = nullptr;
  if (!idx || !out_n) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  uint64_t bits = 0;
  EncRowsWant want;
  want.lines = lines != nullptr;
  CJS_TRY(compress_core(c, d_in, n, level, 0, -1, true, d_out, out_cap, &bits, nullptr, 0, nullptr, stats, &want));
  std::vector<cjs_bz_index_entry> entries; std::vector<uint32_t> newlines;
  const uint64_t end_bit = enc_rows_append(entries, newlines, want.rows.data(), want.rows.size(), ENC_FIRST_BIT, level);
  if (end_bit + 80 != bits) return CJS_E_HIP;            // (the packer's own count of the stream's bits)
  CJS_TRY(enc_tables_make(entries, newlines, end_bit, idx, lines));
  *out_n = (size_t)((bits + 7) / 8);
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_compress_device_range(cjs_ctx* c, const uint8_t* d_in, size_t n, int level, long first_block, long count,
                                               uint8_t* d_out, size_t out_cap, uint64_t* out_bits, uint32_t* block_crcs, long crc_cap,
                                               long* total_blocks, cjs_stats* stats) {
  return compress_core(c, d_in, n, level, first_block, count, false, d_out, out_cap, out_bits, block_crcs, crc_cap, total_blocks, stats);
}

// ------------------------------------------------------------------ one process (or worker thread) per GPU: the phases of a job
// Every rank holds the stream.  Phase 1 makes the boundary tables of the rank's share of the input tiles; the caller exchanges the
// shares (an all-gather, 72 B per 4 KiB tile: the library itself never calls a collective).  Phase 2 walks the block boundaries
// (replicated: O(#blocks) and serial by nature, Q1-Q3) and takes the rank's contiguous range of blocks through the Huffman
// tables; the caller exchanges one cjs_shard_meta per rank.  Phase 3 packs the rank's blocks at their FINAL bit offset: the
// ranks' fragments are disjoint runs of whole 32-bit words of the one .bz2 stream.
extern "C" size_t cjs_bzip2_shard_share_bytes(size_t n, int world) {
  if (world < 1) return 0;
  return Rle1Work::share_bytes(Rle1Work::tiles_per_rank(n, (uint32_t)world));
}
extern "C" int cjs_bzip2_shard_tiles(cjs_ctx* c, const uint8_t* d_in, size_t n, int rank, int world, void* d_share) {
  CJS_GUARD_BEGIN
  if (!c || !d_share || world < 1 || rank < 0 || rank >= world || n > c->max_input) return CJS_E_INVALID_ARG;
  CJS_HIP_TRY(hipSetDevice(c->device));
  c->sh_state = 0;
  const uint32_t tpr = Rle1Work::tiles_per_rank(n, (uint32_t)world);
  const uint64_t t0 = (uint64_t)rank * tpr, Tn = Rle1Work::tiles_for(n);
  if (t0 < Tn) CJS_TRY(rle1_tiles(c->stream, c->rle, d_in, n, (uint32_t)t0, (uint32_t)std::min<uint64_t>(Tn, t0 + tpr), (uint8_t*)d_share, tpr));
  CJS_HIP_TRY(hipStreamSynchronize(c->stream));        // the caller's collective runs on a stream of its own
  c->sh_state = 1;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
// bit length of blocks [0, cnt) of the range and their CRCs folded from 0 -> out[0], out[1]
__global__ void shard_meta_kernel(const uint32_t* __restrict__ bitlen, const uint32_t* __restrict__ block_crc, uint32_t first, uint32_t cnt, uint64_t* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  uint64_t bits = 0; uint32_t c = 0;
  for (uint32_t k = 0; k < cnt; k++) { bits += bitlen[k]; c = ((c << 1) | (c >> 31)) ^ block_crc[first + k]; }
  out[0] = bits; out[1] = c;
}
static void shard_range(uint32_t total, int rank, int world, uint32_t& first, uint32_t& count) {
  const uint32_t share = total ? (total + (uint32_t)world - 1u) / (uint32_t)world : 0u;
  first = std::min<uint64_t>((uint64_t)rank * share, total);
  count = std::min<uint32_t>(share, total - first);
}
int cjs::shard_blocks_impl(cjs_ctx* c, const uint8_t* d_in, size_t n, int level, int rank, int world, const void* d_shares, cjs_shard_meta* meta, cjs_stats* st,
                           EncRowsWant* want) {
  if (!c || !meta || level != c->level || world < 1 || rank < 0 || rank >= world || n > c->max_input || (world > 1 && !d_shares)) return CJS_E_INVALID_ARG;
  if (c->sh_state != 1 && d_shares) return CJS_E_INVALID_ARG;          // phase order
  CJS_HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  c->sh_state = 0;
  CallTimes t;
  CJS_TRY(t.begin(c, st));
  uint32_t nb = 0, last_len = 0;
  if (d_shares) CJS_TRY(rle1_tables_from_shares(s, c->rle, n, (const uint8_t*)d_shares, Rle1Work::tiles_per_rank(n, (uint32_t)world)));
  else if (n) CJS_TRY(rle1_tiles(s, c->rle, d_in, n, 0u, Rle1Work::tiles_for(n), nullptr, 0u));
  CJS_TRY(rle1_walk_run(s, c->rle, d_in, n, &nb, &last_len));
  uint32_t f = 0, cnt = 0;
  shard_range(nb, rank, world, f, cnt);
  CJS_TRY(blocks_through_tables(c, d_in, n, nb, last_len, f, cnt, st, t.stages));
  if (cnt && n && c->side) CJS_HIP_TRY(hipStreamWaitEvent(s, c->ev_join, 0));
  hipLaunchKernelGGL(shard_meta_kernel, dim3(1), dim3(1), 0, s, c->huff.b.bitlen, c->rle.block_crc, f, cnt, c->huff.scalars + 4);
  CJS_HIP_TRY(hipMemcpyAsync(c->h_scalars + 4, c->huff.scalars + 4, 16, hipMemcpyDeviceToHost, s));
  if (want) CJS_TRY(enc_rows_enqueue(c, d_in, n, f, cnt, want->lines));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  if (want) enc_rows_collect(c, cnt, *want);
  meta->bits = c->h_scalars[4]; meta->crc_fold = (uint32_t)c->h_scalars[5];
  meta->total_blocks = nb; meta->first_block = f; meta->blocks = cnt;
  c->sh_nb = nb; c->sh_first = f; c->sh_cnt = cnt; c->sh_state = 2;
  t.end(cnt, n, meta->bits);
  return 0;
}
extern "C" int cjs_bzip2_shard_blocks(cjs_ctx* c, const uint8_t* d_in, size_t n, int level, int rank, int world, const void* d_shares,
                                      cjs_shard_meta* meta, cjs_stats* stats) {
  CJS_GUARD_BEGIN
  return drain_on_error(c, shard_blocks_impl(c, d_in, n, level, rank, world, d_shares, meta, stats));
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
// Packs the context's blocks (phase 2 left them behind) at the stream's bit `start` (the rank's first block; rank 0: 32).
// header / trailer: this rank opens / ends the stream; a rank that does not end it is followed by another rank's blocks.
int cjs::shard_pack_core(cjs_ctx* c, int level, bool header, bool trailer, uint64_t start, uint64_t bits, uint32_t scrc, uint8_t* d_out, size_t out_cap,
                         size_t* frag_off, size_t* frag_len, uint64_t* stream_off) {
  const uint64_t local_start = header ? 32 : (start & 31), end_local = local_start + bits;
  const PackShard ps{scrc, trailer ? 0 : 1};
  uint64_t end_bit = 0;
  CJS_TRY(pack_enqueue(c, PackJob{c->sh_nb, c->sh_first, c->sh_cnt, local_start, level, header, trailer, c->rle.block_crc, c->d_pidx, (uint32_t*)d_out, out_cap & ~(size_t)3, &ps}));
  CJS_TRY(pack_finish(c, &end_bit));
  // the fragment: whole words from the first word that starts inside this rank's bits (rank 0: the stream start) to the word its
  // last bit lands in (completed with the next rank's leading bits), or to the end of the stream
  const uint64_t word0 = header ? 0 : (start >> 5);                             // stream word at d_out[0]
  const uint64_t skip = (!header && (start & 31)) ? 4 : 0;
  const uint64_t end_bytes = trailer ? (end_local + 80 + 7) / 8 : ((end_local + 31) / 32) * 4;
  *frag_off = (size_t)skip; *frag_len = (size_t)(end_bytes > skip ? end_bytes - skip : 0); *stream_off = word0 * 4 + skip;
  return 0;
}
extern "C" int cjs_bzip2_shard_pack(cjs_ctx* c, int level, int rank, int world, const cjs_shard_meta* metas, uint8_t* d_out, size_t out_cap,
                                    size_t* frag_off, size_t* frag_len, uint64_t* stream_off, uint64_t* stream_len) {
  CJS_GUARD_BEGIN
  if (!c || !metas || !frag_off || !frag_len || !stream_off || level != c->level || world < 1 || rank < 0 || rank >= world) return CJS_E_INVALID_ARG;
  if (c->sh_state != 2 || ((uintptr_t)d_out & 3) != 0) return CJS_E_INVALID_ARG;
  const cjs_shard_meta& me = metas[rank];
  if (me.blocks != c->sh_cnt || me.first_block != c->sh_first || me.total_blocks != c->sh_nb) return CJS_E_INVALID_ARG;
  for (int r = 0; r < world; r++) if (metas[r].total_blocks != me.total_blocks) return CJS_E_INVALID_ARG;    // the ranks disagree on the boundaries
  CJS_HIP_TRY(hipSetDevice(c->device));
  uint64_t start, total; uint32_t scrc; int writer;
  shard_layout(metas, world, rank, start, total, scrc, writer);
  if (stream_len) *stream_len = (total + 80 + 7) / 8;
  c->sh_state = 0;
  if (rank && !me.blocks) { *frag_off = 0; *frag_len = 0; *stream_off = (total + 80 + 7) / 8; return 0; }      // nothing of the stream lands here
  return shard_pack_core(c, level, rank == 0, rank == writer, start, me.bits, scrc, d_out, out_cap, frag_off, frag_len, stream_off);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
