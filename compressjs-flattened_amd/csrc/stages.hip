// stages.hip — stage-level entry points of the compress pipeline (host buffers; the parity tests use them to localise a
// mismatch): every call carves a workspace of its own, runs one stage on a stream of its own and copies the stage's output back.
#include "cjs_internal.h"
#include "host.h"
#include "rle1.h"
#include "crc.h"
#include "mtf.h"
#include "huff.h"
#include <algorithm>
#include <vector>

using namespace cjs;

extern "C" int cjs_stage_bwt(const uint8_t* in, size_t n, int block_len, int cyclic, uint8_t* out, int32_t* pidx, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (n == 0) return 0;
  if (block_len <= 0) return CJS_E_INVALID_ARG;
  const uint32_t stride = (uint32_t)block_len;
  const uint32_t nb = (uint32_t)((n + stride - 1) / stride);
  const uint32_t n_last = (uint32_t)(n - (size_t)(nb - 1) * stride);
  Arena arena;
  CJS_TRY(arena.init(BwtWork::bytes_needed(n) + 2 * ((n + 511) & ~(size_t)255) + 4 * (size_t)nb + 8192));
  BwtWork w;
  CJS_TRY(w.carve(arena, n));
  uint8_t* d_T = arena.take<uint8_t>(n);
  uint8_t* d_U = arena.take<uint8_t>(n);
  uint32_t* d_p = arena.take<uint32_t>(nb);
  if (!d_T || !d_U || !d_p) return CJS_E_OUT_OF_MEMORY;
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  CJS_HIP_TRY(hipMemcpyAsync(d_T, in, n, hipMemcpyHostToDevice, s));
  CJS_TRY(bwt_run(s, w, d_T, nb, stride, n_last, cyclic != 0, d_U, d_p, Opts(opts).stats));
  CJS_HIP_TRY(hipMemcpyAsync(out, d_U, n, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(pidx, d_p, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// Blocks of different lengths, one per slot of `stride` bytes: the geometry of the batched compressor (batch.hip, run_sub), which
// instantiates every templated kernel of the sort a second time and sorts round 1 unsegmented, with a depth that follows nb.
extern "C" int cjs_stage_bwt_var(const uint8_t* blocks, uint32_t nb, uint32_t stride, const uint32_t* len, uint8_t* out, int32_t* pidx,
                                 const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (nb == 0 || nb > 65535 || stride == 0 || stride % 16 != 0) return CJS_E_INVALID_ARG;      // (run_list only makes such strides)
  for (uint32_t k = 0; k < nb; k++) if (len[k] == 0 || len[k] > stride) return CJS_E_INVALID_ARG;      // the kernels read len - 1
  const size_t e = (size_t)nb * stride;
  if (!bwt_admits(e, stride)) return CJS_E_INVALID_ARG;
  Arena arena;
  CJS_TRY(arena.init(BwtWork::bytes_needed(e) + 2 * ((e + 16 + 511) & ~(size_t)255) + 8 * (size_t)nb + 8192));
  BwtWork w;
  CJS_TRY(w.carve(arena, e));
  uint8_t* d_T = arena.take<uint8_t>(e + 16);             // 16 bytes of slack behind the text and the output, as run_sub carves them
  uint8_t* d_U = arena.take<uint8_t>(e + 16);
  uint32_t* d_p = arena.take<uint32_t>(nb);
  uint32_t* d_len = arena.take<uint32_t>(nb);
  if (!d_T || !d_U || !d_p || !d_len) return CJS_E_OUT_OF_MEMORY;
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  CJS_HIP_TRY(hipMemcpyAsync(d_T, blocks, e, hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_len, len, 4 * (size_t)nb, hipMemcpyHostToDevice, s));
  CJS_TRY(bwt_run_var(s, w, d_T, nb, stride, d_len, d_U, d_p));
  CJS_HIP_TRY(hipMemcpyAsync(out, d_U, e, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(pidx, d_p, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// Stage 0 over one stream with a block capacity of the caller's choice: `cap` is a run-time argument of every kernel of the stage,
// and a small one puts thousands of block boundaries, each at another chunk phase and subtile offset, into an input of a few
// tiles.  world > 1 makes the tile tables share by share, as the ranks of a sharded job do (pipeline.hip, cjs_bzip2_shard_tiles /
// shard_blocks_impl), into one buffer laid out as their all-gather leaves it; range_blocks > 0 carves the workspace for that
// many blocks per rle1_finish call and takes the blocks through it window by window, as the streaming compressor does.
// work_fill >= 0: the workspace, the share buffer and d_blocks are filled with that byte first (the product reuses them).
//
// The floor of cap is 2.  Rle1Work::max_blocks_for divides by cap * 4 / 5, which is 0 for cap == 1.  Nothing else in the stage
// asks for more: run_fill_input and emitted_fresh hold from cap 1 on (rem == 0 only from cap 5 on, where q >= 1);
// max_segs_for(cap) covers the 51 input bytes per output byte of a block at every cap (a block of cap < 5 ends within its
// first four bytes of a run); subpre counts the bytes of one tile (at most 5120) whatever the cap; and the walk's
// speculation needs two targets never to fall on one input byte, which holds because a byte emits at most 2 <= cap bytes.
// The ceiling is the product's largest capacity (level 9).  rle1_finish launches one row of CRC workgroups per block of a
// window, so a window of more than 65535 blocks is refused as well.
constexpr uint32_t RLE1_CAP_FLOOR = 2, RLE1_CAP_CEIL = 9 * 100000 - 19;
extern "C" int cjs_stage_rle1_cap(const uint8_t* in, size_t n, uint32_t cap, uint32_t world, uint32_t range_blocks, int work_fill,
                                  uint8_t* blocks, size_t blocks_cap, uint32_t* block_len, uint32_t* block_crc, uint64_t* block_start,
                                  uint64_t* block_end, long cap_blocks, long* nblocks, uint32_t* last_len, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (cap < RLE1_CAP_FLOOR || cap > RLE1_CAP_CEIL || world == 0 || world > 65535 || !nblocks) return CJS_E_INVALID_ARG;
  *nblocks = 0;
  if (last_len) *last_len = 0;
  if (n == 0) return 0;
  const size_t maxb = Rle1Work::max_blocks_for(n, cap);
  const size_t rows = range_blocks ? std::min<size_t>(range_blocks, maxb) : maxb;      // blocks per rle1_finish call
  if (rows > 65535) return CJS_E_INVALID_ARG;
  const uint32_t Tn = Rle1Work::tiles_for(n), tpr = Rle1Work::tiles_per_rank(n, world);
  const size_t share = Rle1Work::share_bytes(tpr), shares = world > 1 ? share * world : 0;
  Arena arena;
  CJS_TRY(arena.init(Rle1Work::bytes_needed(n, cap, rows) + n + rows * cap + shares + 65536));
  Rle1Work w;
  CJS_TRY(w.carve(arena, n, cap, rows));
  uint8_t* d_blocks = arena.take<uint8_t>(rows * cap);
  uint8_t* d_shares = shares ? arena.take<uint8_t>(shares) : nullptr;
  const size_t fill_end = arena.used;                      // workspace, block rows and shares are arena.base[0 .. fill_end)
  uint8_t* d_in = arena.take<uint8_t>(n);
  if (!d_in || !d_blocks || (shares && !d_shares)) return CJS_E_OUT_OF_MEMORY;
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  if (work_fill >= 0) CJS_HIP_TRY(hipMemsetAsync(arena.base, work_fill & 0xFF, fill_end, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_in, in, n, hipMemcpyHostToDevice, s));
  uint32_t nb = 0, ll = 0;
  if (world == 1) CJS_TRY(rle1_run(s, w, d_in, n, &nb, &ll));
  else {
    for (uint32_t r = 0; r < world; r++) {                 // every rank in turn; the ranks behind the last tile have no share to make
      const uint64_t t0 = (uint64_t)r * tpr;
      if (t0 < Tn) CJS_TRY(rle1_tiles(s, w, d_in, n, (uint32_t)t0, (uint32_t)std::min<uint64_t>(Tn, t0 + tpr), d_shares + (size_t)r * share, tpr));
    }
    CJS_TRY(rle1_tables_from_shares(s, w, n, d_shares, tpr));
    CJS_TRY(rle1_walk_run(s, w, d_in, n, &nb, &ll));
  }
  *nblocks = (long)nb;
  if (last_len) *last_len = ll;
  if (nb > maxb) return CJS_E_HIP;                          // (the walk counted past its table: max_blocks_for is no bound)
  if ((long)nb > cap_blocks || (size_t)nb * cap > blocks_cap) return CJS_E_OUTPUT_TOO_SMALL;
  for (uint32_t first = 0; first < nb; first += (uint32_t)rows) {
    const uint32_t cnt = (uint32_t)std::min<size_t>(rows, nb - first);
    CJS_TRY(rle1_finish(s, w, d_in, n, first, cnt, d_blocks));
    CJS_HIP_TRY(hipMemcpyAsync(blocks + (size_t)first * cap, d_blocks, (size_t)cnt * cap, hipMemcpyDeviceToHost, s));
    CJS_HIP_TRY(hipStreamSynchronize(s));
  }
  if (nb) {
    std::vector<RleBlock> hb(nb);
    CJS_HIP_TRY(hipMemcpy(hb.data(), w.blocks, sizeof(RleBlock) * nb, hipMemcpyDeviceToHost));
    CJS_HIP_TRY(hipMemcpy(block_len, w.block_len, 4 * (size_t)nb, hipMemcpyDeviceToHost));
    CJS_HIP_TRY(hipMemcpy(block_crc, w.block_crc, 4 * (size_t)nb, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < nb; k++) { block_start[k] = hb[k].s; if (block_end) block_end[k] = hb[k].e; }
  }
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_stage_rle1(const uint8_t* in, size_t n, int level, uint8_t* blocks, size_t blocks_cap,
                              uint32_t* block_len, uint32_t* block_crc, uint64_t* block_start, long cap_blocks, long* nblocks,
                              const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (level < 1 || level > 9) return CJS_E_BAD_LEVEL;
  return cjs_stage_rle1_cap(in, n, (uint32_t)level * 100000u - 19u, 1u, 0u, -1, blocks, blocks_cap, block_len, block_crc, block_start, nullptr,
                            cap_blocks, nblocks, nullptr, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// The three kernels of rle1_batch.hip, each on its own and each with exactly the arrays of the caller (none of batch.hip's host
// logic between them): rle1_batch_len over all `count` inputs in[se[2k] .. se[2k+1]); rle1_batch_walk over the inputs item[0 ..
// nitem) with the block slots tbase[] grants them, into a table of table_slots >= tbase[nitem] entries; rle1_batch_materialize
// and, as run_sub calls it right behind, crc_ranges over the nmat blocks of the caller's table (s / e relative to `in`).  The
// walk's table, nblk[] and the rows are filled with work_fill first, so that what a kernel left untouched can be told apart.
extern "C" int cjs_stage_rle1_batch(const uint8_t* in, size_t in_n, const uint64_t* se, uint32_t count, uint32_t cap, int work_fill,
                                    uint64_t* len2, const uint32_t* item, const uint32_t* tbase, uint32_t nitem, uint32_t table_slots,
                                    uint64_t* walk_s, uint64_t* walk_e, uint32_t* walk_len, uint32_t* nblk, const uint64_t* mat_s,
                                    const uint64_t* mat_e, const uint32_t* mat_len, uint32_t nmat, uint32_t stride, uint8_t* rows,
                                    uint32_t* row_crc, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (cap < RLE1_CAP_FLOOR || cap > RLE1_CAP_CEIL || count > (1u << 20) || nitem > (1u << 20) || table_slots > (1u << 24) || nmat > 65535) return CJS_E_INVALID_ARG;
  if (nitem && !count) return CJS_E_INVALID_ARG;
  for (uint32_t k = 0; k < count; k++) if (se[2 * k] > se[2 * k + 1] || se[2 * k + 1] > in_n) return CJS_E_INVALID_ARG;
  for (uint32_t j = 0; j < nitem; j++) if (item[j] >= count || tbase[j] > tbase[j + 1]) return CJS_E_INVALID_ARG;
  if (nitem && tbase[nitem] > table_slots) return CJS_E_INVALID_ARG;
  if (nmat && stride == 0) return CJS_E_INVALID_ARG;
  size_t longest = 0;
  for (uint32_t j = 0; j < nmat; j++) {
    if (mat_s[j] > mat_e[j] || mat_e[j] > in_n || mat_len[j] > stride) return CJS_E_INVALID_ARG;
    longest = std::max<size_t>(longest, mat_e[j] - mat_s[j]);
  }
  if (!count && !nmat) return 0;
  const size_t segs = crc_segs_for(longest);
  Arena arena;
  CJS_TRY(arena.init(in_n + 16 + 24 * (size_t)count + 8 * ((size_t)nitem + 1) + sizeof(RleBlock) * ((size_t)table_slots + nmat) +
                     (size_t)nmat * (stride + 4 * segs + 4) + 64 + 16 * 256 + 65536));
  uint8_t* d_in = arena.take<uint8_t>(in_n + 16);          // (crc_ranges loads whole 16-byte words around a range)
  uint64_t* d_se = arena.take<uint64_t>(2 * (size_t)count);
  uint64_t* d_len2 = arena.take<uint64_t>(count);
  uint32_t* d_item = arena.take<uint32_t>(nitem);
  uint32_t* d_tbase = arena.take<uint32_t>((size_t)nitem + 1);
  uint32_t* d_nblk = arena.take<uint32_t>(nitem);
  RleBlock* d_tab = arena.take<RleBlock>(table_slots);
  RleBlock* d_rb = arena.take<RleBlock>(nmat);
  uint8_t* d_rows = arena.take<uint8_t>((size_t)nmat * stride);
  uint32_t* d_seg = arena.take<uint32_t>((size_t)nmat * segs);
  uint32_t* d_crc = arena.take<uint32_t>(nmat);
  uint32_t* d_nb = arena.take<uint32_t>(16);
  if (!d_in || !d_se || !d_len2 || !d_item || !d_tbase || !d_nblk || !d_tab || !d_rb || !d_rows || !d_seg || !d_crc || !d_nb) return CJS_E_OUT_OF_MEMORY;
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  CJS_HIP_TRY(hipMemsetAsync(arena.base, work_fill & 0xFF, arena.used, s));
  if (in_n) CJS_HIP_TRY(hipMemcpyAsync(d_in, in, in_n, hipMemcpyHostToDevice, s));
  if (count) {
    CJS_HIP_TRY(hipMemcpyAsync(d_se, se, 16 * (size_t)count, hipMemcpyHostToDevice, s));
    CJS_TRY(rle1_batch_len(s, d_in, d_se, count, cap, d_len2));
    CJS_HIP_TRY(hipMemcpyAsync(len2, d_len2, 8 * (size_t)count, hipMemcpyDeviceToHost, s));
  }
  std::vector<RleBlock> tab(table_slots);
  if (nitem) {
    CJS_HIP_TRY(hipMemcpyAsync(d_item, item, 4 * (size_t)nitem, hipMemcpyHostToDevice, s));
    CJS_HIP_TRY(hipMemcpyAsync(d_tbase, tbase, 4 * ((size_t)nitem + 1), hipMemcpyHostToDevice, s));
    CJS_TRY(rle1_batch_walk(s, d_in, d_se, d_item, d_tbase, nitem, cap, d_tab, d_nblk));
    CJS_HIP_TRY(hipMemcpyAsync(nblk, d_nblk, 4 * (size_t)nitem, hipMemcpyDeviceToHost, s));
  }
  if (table_slots) CJS_HIP_TRY(hipMemcpyAsync(tab.data(), d_tab, sizeof(RleBlock) * table_slots, hipMemcpyDeviceToHost, s));
  if (nmat) {
    std::vector<RleBlock> rb(nmat);
    for (uint32_t j = 0; j < nmat; j++) { rb[j] = RleBlock{}; rb[j].s = mat_s[j]; rb[j].e = mat_e[j]; rb[j].len = mat_len[j]; }
    const uint32_t nbv = nmat;
    CJS_HIP_TRY(hipMemcpyAsync(d_rb, rb.data(), sizeof(RleBlock) * nmat, hipMemcpyHostToDevice, s));
    CJS_HIP_TRY(hipMemcpyAsync(d_nb, &nbv, 4, hipMemcpyHostToDevice, s));
    CJS_HIP_TRY(hipStreamSynchronize(s));                  // (rb and nbv are this scope's)
    CJS_TRY(rle1_batch_materialize(s, d_in, d_rb, nmat, stride, d_rows));
    CJS_TRY(crc_ranges(s, d_in, d_rb, d_nb, nmat, (uint32_t)segs, d_seg, d_crc));
    CJS_HIP_TRY(hipMemcpyAsync(rows, d_rows, (size_t)nmat * stride, hipMemcpyDeviceToHost, s));
    if (row_crc) CJS_HIP_TRY(hipMemcpyAsync(row_crc, d_crc, 4 * (size_t)nmat, hipMemcpyDeviceToHost, s));
  }
  CJS_HIP_TRY(hipStreamSynchronize(s));
  for (uint32_t q = 0; q < table_slots; q++) { walk_s[q] = tab[q].s; walk_e[q] = tab[q].e; walk_len[q] = tab[q].len; }
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_stage_mtf(const uint8_t* U, const uint8_t* blocks, size_t n, int block_len, uint16_t* A, uint32_t* npos,
                             uint32_t* freq, uint32_t* alphabet, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  (void)blocks;   // the used-symbol set of a block equals that of its BWT (a permutation of it)
  CJS_TRY(select_device(opts));
  if (n == 0) return 0;
  if (block_len <= 0) return CJS_E_INVALID_ARG;
  const uint32_t stride = (uint32_t)block_len, nb = (uint32_t)((n + stride - 1) / stride);
  Arena arena;
  CJS_TRY(arena.init(MtfWork::bytes_needed(nb, stride) + (size_t)nb * stride + 4 * (size_t)nb + 65536));
  MtfWork w;
  CJS_TRY(w.carve(arena, nb, stride));
  uint8_t* d_U = arena.take<uint8_t>((size_t)nb * stride);
  uint32_t* d_len = arena.take<uint32_t>(nb);
  if (!d_U || !d_len) return CJS_E_OUT_OF_MEMORY;
  std::vector<uint32_t> lens(nb, stride);
  lens[nb - 1] = (uint32_t)(n - (size_t)(nb - 1) * stride);
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  CJS_HIP_TRY(hipMemcpy(d_U, U, n, hipMemcpyHostToDevice));
  CJS_HIP_TRY(hipMemcpy(d_len, lens.data(), 4 * (size_t)nb, hipMemcpyHostToDevice));
  CJS_TRY(mtf_run(s, w, d_U, nb, d_len));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  std::vector<uint32_t> hnpos(nb);
  CJS_HIP_TRY(hipMemcpy(hnpos.data(), w.b.npos, 4 * (size_t)nb, hipMemcpyDeviceToHost));
  CJS_HIP_TRY(hipMemcpy(freq, w.b.freq, 4 * 258 * (size_t)nb, hipMemcpyDeviceToHost));
  CJS_HIP_TRY(hipMemcpy(alphabet, w.b.asz, 4 * (size_t)nb, hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < nb; k++) {
    npos[k] = hnpos[k];
    CJS_HIP_TRY(hipMemcpy(A + (size_t)k * (stride + 1), w.b.A + (size_t)k * w.b.a_stride, 2 * (size_t)hnpos[k], hipMemcpyDeviceToHost));
  }
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// Blocks of different lengths, one per slot of `stride` bytes, as both callers of mtf_run hand them over: the pipeline's rows start
// at odd addresses (stride = level * 100000 - 19), the batch compressor's at multiples of 16.  What the slots hold behind a block's
// end is the caller's (hole bytes in `blocks`), and the whole workspace is filled with `work_fill` before the run: the product
// reuses its workspace between calls, so every kernel meets stale heads, lists and segment keys there.
// The head kernels read aligned 32-bit words around a thread's first byte p0 < len: al[-1] .. al[4], the last byte of which lies
// at most 16 bytes behind p0, so at most 16 bytes behind a block's last byte.  Inside the array that is the next slot; behind the
// last slot batch.hip has its 16 bytes of slack (and, with rows a multiple of 16, never reads past the row), and pipeline.hip's
// d_U is followed in its arena by d_pidx and 64 KiB of slack (Arena::take rounds to 256): both cover the reach.  d_U is carved
// here as batch.hip carves it.
extern "C" int cjs_stage_mtf_var(const uint8_t* blocks, uint32_t nb, uint32_t stride, const uint32_t* len, int work_fill, uint16_t* A,
                                 uint32_t* npos, uint32_t* freq, uint32_t* alphabet, uint8_t* alist, uint32_t* nheads, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (nb == 0 || nb > 65535 || stride == 0) return CJS_E_INVALID_ARG;
  if (((size_t)stride + 4095) / 4096 > 1024) return CJS_E_INVALID_ARG;      // mtf_run scans a block's tile counts in one workgroup
  for (uint32_t k = 0; k < nb; k++) if (len[k] == 0 || len[k] > stride) return CJS_E_INVALID_ARG;
  const size_t e = (size_t)nb * stride;
  Arena arena;
  const size_t wbytes = MtfWork::bytes_needed(nb, stride);
  CJS_TRY(arena.init(wbytes + e + 16 + 4 * (size_t)nb + 65536));
  MtfWork w;
  CJS_TRY(w.carve(arena, nb, stride));
  const size_t wend = arena.used;                          // the workspace is arena.base[0 .. wend)
  uint8_t* d_U = arena.take<uint8_t>(e + 16);
  uint32_t* d_len = arena.take<uint32_t>(nb);
  if (!d_U || !d_len) return CJS_E_OUT_OF_MEMORY;
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  CJS_HIP_TRY(hipMemsetAsync(arena.base, work_fill & 0xFF, wend, s));
  CJS_HIP_TRY(hipMemsetAsync(d_U + e, work_fill & 0xFF, 16, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_U, blocks, e, hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_len, len, 4 * (size_t)nb, hipMemcpyHostToDevice, s));
  CJS_TRY(mtf_run(s, w, d_U, nb, d_len));                  // (refuses the strides whose tile counts it cannot scan)
  std::vector<uint32_t> hnpos(nb);
  CJS_HIP_TRY(hipMemcpyAsync(hnpos.data(), w.b.npos, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(freq, w.b.freq, 4 * 258 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(alphabet, w.b.asz, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(alist, w.b.alist, 256 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(nheads, w.b.nheads, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  for (uint32_t k = 0; k < nb; k++) {
    if (hnpos[k] == 0 || hnpos[k] > stride + 1) return CJS_E_OUTPUT_TOO_SMALL;       // (a row of A holds stride + 1 symbols)
    CJS_HIP_TRY(hipMemcpyAsync(A + (size_t)k * ((size_t)stride + 1), w.b.A + (size_t)k * w.b.a_stride, 2 * (size_t)hnpos[k], hipMemcpyDeviceToHost, s));
  }
  CJS_HIP_TRY(hipStreamSynchronize(s));
  for (uint32_t k = 0; k < nb; k++) npos[k] = hnpos[k];
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_stage_huff(const uint16_t* A, uint32_t npos, uint32_t alphabet, uint8_t* selectors, uint8_t* lengths,
                              uint32_t* ngroups, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (npos == 0 || alphabet == 0 || alphabet > 256) return CJS_E_INVALID_ARG;
  const uint32_t stride = npos;    // any stride >= npos-1 works for the selector buffers
  Arena arena;
  CJS_TRY(arena.init(HuffWork::bytes_needed(1, stride) + 2 * (size_t)npos + 4096 * 4 + 65536));
  HuffWork w;
  const int rc = w.carve(arena, 1, stride);
  uint16_t* d_A = arena.take<uint16_t>(npos);
  uint32_t* d_misc = arena.take<uint32_t>(2 + 258);
  uint8_t* d_alist = arena.take<uint8_t>(256);
  std::vector<uint32_t> misc(2 + 258, 0);
  misc[0] = npos; misc[1] = alphabet;
  for (uint32_t i = 0; i < npos; i++) { if (A[i] > alphabet + 1) return CJS_E_INVALID_ARG; misc[2 + A[i]]++; }
  CJS_TRY(rc);
  if (!d_A || !d_misc || !d_alist) return CJS_E_OUT_OF_MEMORY;
  uint8_t al[256]; for (int i = 0; i < 256; i++) al[i] = (uint8_t)i;
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  CJS_HIP_TRY(hipMemcpy(d_A, A, 2 * (size_t)npos, hipMemcpyHostToDevice));
  CJS_HIP_TRY(hipMemcpy(d_misc, misc.data(), 4 * misc.size(), hipMemcpyHostToDevice));
  CJS_HIP_TRY(hipMemcpy(d_alist, al, 256, hipMemcpyHostToDevice));
  CJS_TRY(huff_tables_run(s, w, 1, SymRows{d_A, npos, d_misc, d_misc + 1, d_misc + 2, d_alist}));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  const uint32_t nsel = groups_for(npos);
  CJS_HIP_TRY(hipMemcpy(selectors, w.b.sel, nsel, hipMemcpyDeviceToHost));
  CJS_HIP_TRY(hipMemcpy(lengths, w.b.lens, lens_row_bytes(), hipMemcpyDeviceToHost));
  CJS_HIP_TRY(hipMemcpy(ngroups, w.b.ngroups, 4, hipMemcpyDeviceToHost));
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_stage_huff_blocks(const uint16_t* A, size_t a_stride, uint32_t nb, const uint32_t* npos, const uint32_t* alphabet,
                                     const uint8_t* used, const uint32_t* block_crc, const uint32_t* pidx, int path,
                                     uint32_t* ngroups, uint8_t* selectors, uint8_t* lengths, uint8_t* bits, size_t bits_stride,
                                     uint64_t* nbits, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (nb == 0 || nb > 65535 || a_stride == 0 || (path != HUFF_AUTO && path != HUFF_PER_BLOCK && path != HUFF_CHAIN)) return CJS_E_INVALID_ARG;
  // the blocks' symbol counts (the MTF stage's freq[]) and the checks the kernels rely on: symbols index tables of asz + 2 entries
  std::vector<uint32_t> freq((size_t)nb * 258, 0);
  std::vector<uint8_t> alist((size_t)nb * 256, 0);
  uint32_t max_npos = 0;
  for (uint32_t k = 0; k < nb; k++) {
    const uint32_t n = npos[k], asz = alphabet[k];
    if (n == 0 || n > a_stride || n > 50u * 32767u || asz == 0 || asz > 256) return CJS_E_INVALID_ARG;     // (15-bit selector count)
    for (uint32_t i = 0; i < asz; i++) {
      if (i && used[(size_t)k * 256 + i] <= used[(size_t)k * 256 + i - 1]) return CJS_E_INVALID_ARG;     // ascending, distinct
      alist[(size_t)k * 256 + i] = used[(size_t)k * 256 + i];
    }
    const uint16_t* a = A + (size_t)k * a_stride;
    for (uint32_t i = 0; i < n; i++) { if (a[i] > asz + 1) return CJS_E_INVALID_ARG; freq[(size_t)k * 258 + a[i]]++; }
    max_npos = std::max(max_npos, n);
  }
  // device rows as the pipeline carves them: a block of up to `stride` bytes yields up to stride + 1 symbols
  const uint32_t stride = max_npos > 1 ? max_npos - 1 : 1;
  const size_t das = MtfWork::a_stride_for(stride);
  Arena arena;
  CJS_TRY(arena.init(HuffWork::bytes_needed(nb, stride) + 2 * das * nb + (size_t)nb * (258 * 4 + 256 + 5 * 4 + 8) + 16 * 256 + 65536));
  HuffWork w;
  CJS_TRY(w.carve(arena, nb, stride));
  uint16_t* d_A = arena.take<uint16_t>(das * nb);
  uint32_t* d_npos = arena.take<uint32_t>(nb);
  uint32_t* d_asz = arena.take<uint32_t>(nb);
  uint32_t* d_freq = arena.take<uint32_t>((size_t)nb * 258);
  uint8_t* d_alist = arena.take<uint8_t>((size_t)nb * 256);
  uint32_t* d_crc = arena.take<uint32_t>(nb);
  uint32_t* d_pidx = arena.take<uint32_t>(nb);
  uint64_t* d_soff = arena.take<uint64_t>(nb);
  uint32_t* d_slen = arena.take<uint32_t>(nb);
  if (!d_A || !d_npos || !d_asz || !d_freq || !d_alist || !d_crc || !d_pidx || !d_soff || !d_slen) return CJS_E_OUT_OF_MEMORY;
  const SymRows rows{d_A, das, d_npos, d_asz, d_freq, d_alist};
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  CJS_HIP_TRY(hipMemsetAsync(d_A, 0, 2 * das * nb, s));
  CJS_HIP_TRY(hipMemsetAsync(w.b.lens, 0, (size_t)nb * lens_row_bytes(), s));
  CJS_HIP_TRY(hipMemcpy2DAsync(d_A, 2 * das, A, 2 * a_stride, 2 * (size_t)max_npos, nb, hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_npos, npos, 4 * (size_t)nb, hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_asz, alphabet, 4 * (size_t)nb, hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_freq, freq.data(), 4 * freq.size(), hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_alist, alist.data(), alist.size(), hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_crc, block_crc, 4 * (size_t)nb, hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(d_pidx, pidx, 4 * (size_t)nb, hipMemcpyHostToDevice, s));
  CJS_TRY(huff_tables_run(s, w, nb, rows, path));
  // the blocks' bare bit strings (no stream header / trailer), each from bit 0 at a 4-byte aligned offset
  CJS_TRY(huff_batch_offsets_run(s, w, nb, 0, 0, d_soff, d_slen));
  uint64_t total = 0;
  CJS_HIP_TRY(hipMemcpyAsync(&total, w.scalars, 8, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  Arena oarena;
  CJS_TRY(oarena.init(total + 4096));
  uint32_t* d_out = oarena.take<uint32_t>((total + 16 + 3) / 4);
  if (!d_out) return CJS_E_OUT_OF_MEMORY;
  CJS_HIP_TRY(hipMemsetAsync(d_out, 0, total + 16, s));
  CJS_TRY(huff_batch_pack_run(s, w, rows, PackJob{nb, 0, nb, 0, 9, false, false, d_crc, d_pidx, d_out, 0}, d_soff));
  std::vector<uint64_t> soff(nb);
  std::vector<uint32_t> slen(nb), blen(nb);
  CJS_HIP_TRY(hipMemcpyAsync(soff.data(), d_soff, 8 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(slen.data(), d_slen, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(blen.data(), w.b.bitlen, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(ngroups, w.b.ngroups, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpyAsync(lengths, w.b.lens, (size_t)nb * lens_row_bytes(), hipMemcpyDeviceToHost, s));
  const size_t hsel = groups_for(a_stride);
  CJS_HIP_TRY(hipMemcpy2DAsync(selectors, hsel, w.b.sel, w.b.sel_stride, groups_for((size_t)max_npos), nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  for (uint32_t k = 0; k < nb; k++) if (slen[k] > bits_stride) return CJS_E_INVALID_ARG;      // (nothing of the bits written yet)
  for (uint32_t k = 0; k < nb; k++) {
    CJS_HIP_TRY(hipMemcpyAsync(bits + (size_t)k * bits_stride, (const uint8_t*)d_out + soff[k], slen[k], hipMemcpyDeviceToHost, s));
    nbits[k] = blen[k];
  }
  CJS_HIP_TRY(hipStreamSynchronize(s));
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
