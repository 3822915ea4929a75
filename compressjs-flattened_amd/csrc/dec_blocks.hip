// dec_blocks.hip — steps 1 and 2 of the Bzip2 decoder (the map: decode.hip): the magic scan, the block decode in stages (bz_stage2.h,
// single-stream form; the move-to-front kernels; the row packer) and phase A of the engine (dec_engine.h), which runs them over a
// share's bytes.
#include "dec_engine.h"
#include "prims.hpp"
#include <stdlib.h>

using namespace cjs;

namespace cjs {

// ---------------------------------------------------------------- 1. magic scan
// `in` is addressed by absolute stream byte; bytes [byte0, byte1) are tested as candidate starts, reads stay below n
__global__ __launch_bounds__(256) void bz_magic_scan(const uint8_t* __restrict__ in, uint64_t byte0, uint64_t byte1, uint64_t n, Cand* __restrict__ out, uint32_t cap,
                                                     uint32_t* __restrict__ count) {
  const uint64_t byte = byte0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (byte >= byte1 || byte + 6 > n) return;
  uint64_t w = 0;
  for (int i = 0; i < 7; i++) w = (w << 8) | (byte + i < n ? in[byte + i] : 0);      // 56 bits
  for (int b = 0; b < 8; b++) {
    if (byte * 8 + b + 48 > n * 8) break;
    const uint64_t v = (w >> (8 - b)) & 0xFFFFFFFFFFFFull;
    if (v == MAGIC_BLOCK || v == MAGIC_END) {
      const uint32_t idx = atomicAdd(count, 1u);
      if (idx < cap) { out[idx].bit = byte * 8 + b; out[idx].kind = v == MAGIC_END; out[idx].pad = 0; }
    }
  }
}
__device__ uint64_t g_dec_clk[8];      // phase clock of candidate 0 (CJS_DEBUG): 100 MHz ticks

// stage 2b's kernels, single-stream form (the batch form: batch_dec.hip)
#define BZ_BATCH 0
#include "bz_stage2.h"
#undef BZ_BATCH


constexpr uint32_t MT_TILE = 256;
// grid = (tile groups, rows of a slab): rows come in slabs of <= 65535 (grid.y), and a grid may not exceed 2^32 threads in all
__global__ __launch_bounds__(256) void bz_mtf_tiles(uint8_t* __restrict__ ops_all, uint32_t ops_stride, const uint32_t* __restrict__ nops_all,
                                                    uint8_t* __restrict__ pl_all, uint32_t tiles_per_row, uint32_t row0) {
  const uint32_t row = row0 + blockIdx.y, t = blockIdx.x * 4u + (threadIdx.x >> 6);
  const int lane = lane_id();
  const uint32_t nops = nops_all[row];
  if ((size_t)t * MT_TILE >= nops) return;
  const uint32_t len = nops - t * MT_TILE < MT_TILE ? nops - t * MT_TILE : MT_TILE;
  uint32_t* opw = reinterpret_cast<uint32_t*>(ops_all + (size_t)row * ops_stride + (size_t)t * MT_TILE);
  const uint32_t opsreg = opw[lane];
  uint32_t L = (uint32_t)(4 * lane) * 0x01010101u + 0x03020100u;      // identity list: slot 4*lane+b holds 4*lane+b
  uint32_t qreg = 0;
  const int lane4m1 = 4 * lane - 1;
#pragma unroll 1
  for (uint32_t j = 0; j < len; j++) {
    const uint32_t k = ((uint32_t)__builtin_amdgcn_readlane(opsreg, j >> 2) >> (8u * (j & 3u))) & 0xFFu;
    const uint32_t v = ((uint32_t)__builtin_amdgcn_readlane(L, k >> 2) >> (8u * (k & 3u))) & 0xFFu;
    const uint32_t up = __builtin_amdgcn_update_dpp(v << 24, L, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    const uint32_t shifted = __builtin_amdgcn_alignbit(L, up, 24);
    int nbm = (int)k - lane4m1;                                          // bytes of this lane that move one slot up
    nbm = nbm < 0 ? 0 : nbm > 4 ? 4 : nbm;
    const uint32_t m = (uint32_t)((1ull << (8 * nbm)) - 1ull);
    L = (shifted & m) | (L & ~m);
    qreg = (uint32_t)lane == (j >> 2) ? qreg | (v << (8u * (j & 3u))) : qreg;
  }
  opw[lane] = qreg;                                                      // (bytes behind len are scratch: the row has room for a whole tile)
  reinterpret_cast<uint32_t*>(pl_all + ((size_t)row * tiles_per_row + t) * MT_TILE)[lane] = L;
}

// The tiles of a row are chained in chunks of MC_TILES: first every chunk's product of permutations (from the identity), then -- chunk
// by chunk again, all at once -- the start list of the chunk (the row's initial list through the products of the chunks in front) and
// from it the start list of each of its tiles.  (One workgroup walking a row's ~1,300 tiles, two barriers each, took 0.48 ms per 100 MB.)
constexpr uint32_t MC_TILES = 64;
__global__ __launch_bounds__(256) void bz_mtf_chunk_perm(const uint32_t* __restrict__ nops_all, const uint8_t* __restrict__ pl_all, uint32_t tiles_per_row,
                                                         uint8_t* __restrict__ cperm_all, size_t cperm_stride) {
  __shared__ uint8_t sl[256];
  const uint32_t row = blockIdx.y, p = threadIdx.x;
  const uint32_t nt = (nops_all[row] + MT_TILE - 1) / MT_TILE, t0 = blockIdx.x * MC_TILES, t1 = min(t0 + MC_TILES, nt);
  if (t0 >= nt) return;
  const uint8_t* pl = pl_all + (size_t)row * tiles_per_row * MT_TILE;
  uint8_t cur = (uint8_t)p, idx = pl[(size_t)t0 * MT_TILE + p];
  for (uint32_t t = t0; t < t1; t++) {
    const uint8_t nidx = t + 1 < t1 ? pl[(size_t)(t + 1) * MT_TILE + p] : 0;      // the next permutation travels while this one is applied
    sl[p] = cur;
    __syncthreads();
    cur = sl[idx];
    __syncthreads();
    idx = nidx;
  }
  cperm_all[(size_t)row * cperm_stride + (size_t)blockIdx.x * 256 + p] = cur;
}
__global__ __launch_bounds__(256) void bz_mtf_compose(const uint32_t* __restrict__ nops_all, const uint8_t* __restrict__ l0_all, uint8_t* __restrict__ pl_all,
                                                      uint32_t tiles_per_row, const uint8_t* __restrict__ cperm_all, size_t cperm_stride) {
  __shared__ uint8_t sl[256];
  const uint32_t row = blockIdx.y, p = threadIdx.x;
  const uint32_t nt = (nops_all[row] + MT_TILE - 1) / MT_TILE, t0 = blockIdx.x * MC_TILES, t1 = min(t0 + MC_TILES, nt);
  if (t0 >= nt) return;
  uint8_t* pl = pl_all + (size_t)row * tiles_per_row * MT_TILE;
  const uint8_t* cp = cperm_all + (size_t)row * cperm_stride;
  uint8_t cur = l0_all[(size_t)row * 256 + p];
  uint8_t idx = blockIdx.x ? cp[p] : pl[(size_t)t0 * MT_TILE + p];
  for (uint32_t c = 0; c < blockIdx.x; c++) {                                      // the chunks in front
    const uint8_t nidx = c + 1 < blockIdx.x ? cp[(size_t)(c + 1) * 256 + p] : pl[(size_t)t0 * MT_TILE + p];
    sl[p] = cur;
    __syncthreads();
    cur = sl[idx];
    __syncthreads();
    idx = nidx;
  }
  for (uint32_t t = t0; t < t1; t++) {
    const uint8_t nidx = t + 1 < t1 ? pl[(size_t)(t + 1) * MT_TILE + p] : 0;
    sl[p] = cur;
    __syncthreads();
    pl[(size_t)t * MT_TILE + p] = cur;                                            // start list of tile t, in place of its permutation
    cur = sl[idx];
    __syncthreads();
    idx = nidx;
  }
}

__global__ __launch_bounds__(256) void bz_mtf_emit(const uint8_t* __restrict__ q_all, const uint32_t* __restrict__ opoff_all, uint32_t ops_stride,
                                                   const uint32_t* __restrict__ nops_all, const uint8_t* __restrict__ l0_all, const uint8_t* __restrict__ pl_all,
                                                   uint32_t tiles_per_row, uint32_t row0, uint8_t* __restrict__ tt_all, uint32_t dbuf_size) {
  const uint32_t row = row0 + blockIdx.y, t = blockIdx.x;
  const int lane = lane_id();
  const uint32_t nops = nops_all[row];
  if ((size_t)t * MT_TILE >= nops && t) return;
  const uint8_t* q = q_all + (size_t)row * ops_stride;
  const uint32_t* opoff = opoff_all + (size_t)row * ops_stride;
  uint8_t* tt = tt_all + (size_t)row * dbuf_size;
  const uint32_t j = t * MT_TILE + threadIdx.x;
  uint32_t o = 0, gap = 0, byte = 0;
  bool live = j < nops;
  if (live) {
    byte = pl_all[((size_t)row * tiles_per_row + t) * MT_TILE + q[j]];
    o = opoff[j];
    gap = opoff[j + 1] - o - 1u;                            // the zero-rank run behind this op repeats its byte (the list front)
    tt[o] = (uint8_t)byte;
    o++;
  }
  if (live && gap <= 16u) { for (uint32_t x = 0; x < gap; x++) tt[o + x] = (uint8_t)byte; live = false; }
  uint64_t mask = __ballot(live && gap > 16u);
  while (mask) {                                           // long runs: the whole wave fills
    const int l = (int)__builtin_ctzll(mask);
    mask &= mask - 1;
    const uint32_t jo = (uint32_t)__builtin_amdgcn_readlane((int)o, l), jl = (uint32_t)__builtin_amdgcn_readlane((int)gap, l);
    const uint32_t jb = (uint32_t)__builtin_amdgcn_readlane((int)byte, l);
    for (uint32_t x = lane; x < jl; x += 64) tt[jo + x] = (uint8_t)jb;
  }
  if (t == 0 && threadIdx.x < 64) {                        // the run in front of the first op repeats the initial list front
    const uint32_t pre = opoff[0], b0 = l0_all[(size_t)row * 256];
    for (uint32_t x = lane; x < pre; x += 64) tt[x] = (uint8_t)b0;
  }
}

// decoded rows of a batch -> their packed places (phase A with several batches)
struct RowDst { uint64_t dst; uint64_t count; };      // device address of the row's packed place, bytes to copy
__global__ __launch_bounds__(256) void bz_rows_pack(const uint8_t* __restrict__ rows, uint32_t stride, const RowDst* __restrict__ desc) {
  const RowDst d = desc[blockIdx.y];
  uint8_t* __restrict__ dst = reinterpret_cast<uint8_t*>(d.dst);
  const uint32_t cnt = (uint32_t)d.count;
  const uint8_t* __restrict__ src = rows + (size_t)blockIdx.y * stride;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) dst[i] = src[i];
}

// ---------------------------------------------------------------- phase A: upload, candidates, block decode of every candidate in row batches
// Device scratch of a row batch: nr rows of each (RowLayout), used again by every batch.  One batch: ttb, the decoded rows, is the
// share's (phase B's input); several: gdst, the rows' packed places (host copy: gdst_host).  rlim: a batch group's row limits.
struct RowScratch {
  uint8_t *ttb = nullptr, *ops = nullptr, *l0 = nullptr, *pl = nullptr, *sel = nullptr; uint32_t *opoff = nullptr, *nops = nullptr, *gstart = nullptr, *rlim = nullptr;
  BlockOut* bo = nullptr; RowTab* tabs = nullptr; uint16_t* syms = nullptr; RowDst* gdst = nullptr;
  std::vector<RowDst> gdst_host;
  int take(DecShare& S, ShareScratch& q, const RowLayout& L, uint32_t dsz, uint32_t ncand, bool group);
};
// what the steps of phase A hand on
struct ARun {
  DecJob& J; DecShare& S; hipStream_t s;
  ShareScratch q;                                    // (the upload stays with the share)
  size_t up_n; uint32_t nin;                         // uploaded bytes; inputs of a batch group (0: one stream)
  uint32_t cand_cap = 0, ncand = 0, nrows = 0;
  Cand* d_cand = nullptr; uint32_t *d_count = nullptr, *d_bst = nullptr, *d_ben = nullptr;
  uint32_t* d_cend = nullptr;                        // batch: per candidate, its input's end and block size (cend, then cdsz)
  RowLayout L{}; RowScratch R;
};

// the share's bytes at the dword phase of the stream, the zeroed candidate count, a batch group's input bounds
static int upload(ARun& a) {
  DecShare& S = a.S;
  a.cand_cap = a.J.given ? (uint32_t)S.cands.size() + 1u : (uint32_t)((S.hi - S.lo) / 64 + 1024);      // grown to the exact count if a file of tiny streams has more
  uint8_t* d_raw = nullptr;
  CJS_TRY(S.take((void**)&d_raw, a.up_n + 256 + 16));
  CJS_TRY(a.q.take((void**)&a.d_cand, sizeof(Cand) * a.cand_cap));
  CJS_TRY(a.q.take((void**)&a.d_count, 64));
  // keep the dword phase of the stream: the decoders fetch aligned big-endian words by absolute word index
  uint8_t* d_al = d_raw + (S.up_lo & 3u);
  S.d_in = d_al - S.up_lo;
  if (a.J.upload) CJS_TRY(a.J.upload(&S, d_al));                        // (a device source: its own copy or gather)
  else { DEC_HIP(hipMemcpyAsync(d_al, a.J.in + S.up_lo, a.up_n, hipMemcpyHostToDevice, a.s)); S.h2d += a.up_n; }
  DEC_HIP(hipMemsetAsync(a.d_count, 0, 64, a.s));
  if (!a.nin) return 0;
  CJS_TRY(a.q.take((void**)&a.d_bst, 4 * (size_t)a.nin));
  CJS_TRY(a.q.take((void**)&a.d_ben, 4 * (size_t)a.nin));
  DEC_HIP(hipMemcpyAsync(a.d_bst, S.bst.data(), 4 * (size_t)a.nin, hipMemcpyHostToDevice, a.s));
  DEC_HIP(hipMemcpyAsync(a.d_ben, S.ben.data(), 4 * (size_t)a.nin, hipMemcpyHostToDevice, a.s));
  S.h2d += 8 * (size_t)a.nin;
  return 0;
}

// the magic scan into d_cand (room for cand_cap) and the number of magics it met -> a.ncand, with the stream drained
static int scan_and_count(ARun& a) {
  DecShare& S = a.S;
  if (a.nin) launch_magic_scan_batch(a.s, S.d_in, a.d_bst, a.d_ben, a.nin, S.hi, a.d_cand, a.cand_cap, a.d_count);
  else for (uint64_t b0 = S.lo; b0 < S.hi; b0 += 1ull << 31) {         // (slabs: a grid may not exceed 2^32 threads)
    const uint64_t b1 = std::min<uint64_t>(S.hi, b0 + (1ull << 31));
    hipLaunchKernelGGL(bz_magic_scan, dim3((unsigned)((b1 - b0 + 255) / 256)), dim3(256), 0, a.s, S.d_in, b0, b1, S.up_hi, a.d_cand, a.cand_cap, a.d_count);
  }
  a.ncand = 0;
  DEC_HIP(hipMemcpyAsync(&a.ncand, a.d_count, 4, hipMemcpyDeviceToHost, a.s));
  DEC_HIP(hipStreamSynchronize(a.s));
  S.d2h += 4;
  return 0;
}
// The share's candidates, sorted by bit: scanned for, or given (range reads), then vetted by the caller
static int candidates(ARun& a) {
  DecShare& S = a.S;
  if (a.J.given) {
    if (a.J.vet) CJS_TRY(a.J.vet(&S));
    a.ncand = (uint32_t)S.cands.size();
    return 0;
  }
  for (int round = 0; round < 2; round++) {
    if (round) {                                                        // more magics than planned for (many tiny member streams): scan again with room for all
      a.q.drop(a.d_cand);
      a.cand_cap = a.ncand;
      CJS_TRY(a.q.take((void**)&a.d_cand, sizeof(Cand) * a.cand_cap));
      DEC_HIP(hipMemsetAsync(a.d_count, 0, 64, a.s));
    }
    CJS_TRY(scan_and_count(a));
    if (a.ncand <= a.cand_cap) break;
  }
  if (a.ncand > a.cand_cap) return CJS_E_HIP;
  S.cands.resize(a.ncand);
  if (a.ncand) DEC_HIP(hipMemcpy(S.cands.data(), a.d_cand, sizeof(Cand) * a.ncand, hipMemcpyDeviceToHost));
  S.d2h += sizeof(Cand) * (size_t)a.ncand;
  std::sort(S.cands.begin(), S.cands.end(), [](const Cand& x, const Cand& y) { return x.bit < y.bit; });
  S.ncand_seen = a.ncand;
  return 0;
}

// The candidates as the kernels get them: a device source's end-of-stream records, a batch group's per-candidate limits, a row
// number for every block candidate (only they get a row of the decode buffer)
static int number_rows(ARun& a) {
  DecShare& S = a.S;
  const uint32_t ncand = a.ncand;
  if (a.J.eos && ncand) CJS_TRY(a.J.eos(&S));
  if (a.nin && ncand) {                                            // the batch scan left each candidate's input in pad
    std::vector<uint32_t> cend(2 * (size_t)ncand);
    for (uint32_t c = 0; c < ncand; c++) { cend[c] = S.ben[S.cands[c].pad]; cend[ncand + c] = S.bdsz[S.cands[c].pad]; }
    CJS_TRY(a.q.take((void**)&a.d_cend, 8 * (size_t)ncand));
    DEC_HIP(hipMemcpy(a.d_cend, cend.data(), 8 * (size_t)ncand, hipMemcpyHostToDevice));
    S.h2d += 8 * (size_t)ncand;
  }
  a.nrows = 0;
  for (auto& c : S.cands) c.pad = c.kind == 0 ? a.nrows++ : 0u;
  if (ncand) DEC_HIP(hipMemcpy(a.d_cand, S.cands.data(), sizeof(Cand) * ncand, hipMemcpyHostToDevice));
  S.h2d += sizeof(Cand) * (size_t)ncand;
  S.bos.resize(ncand);
  S.tt_ptr.assign(ncand, 0ull);
  return 0;
}

// nr rows of dsz bytes and their stage buffers, a BlockOut per candidate; group: a batch group's row limits as well
int RowScratch::take(DecShare& S, ShareScratch& q, const RowLayout& L, uint32_t dsz, uint32_t ncand, bool group) {
  const size_t nr = L.nr;
  CJS_TRY(L.single ? S.take((void**)&ttb, nr * dsz) : q.take((void**)&ttb, nr * dsz));      // (one batch: the rows are phase B's input)
  CJS_TRY(q.take((void**)&bo, sizeof(BlockOut) * ncand));
  CJS_TRY(q.take((void**)&ops, nr * L.ops_stride));
  CJS_TRY(q.take((void**)&opoff, 4 * nr * L.ops_stride));
  CJS_TRY(q.take((void**)&l0, nr * 256));
  CJS_TRY(q.take((void**)&pl, nr * L.ops_stride));
  CJS_TRY(q.take((void**)&nops, 4 * nr));
  CJS_TRY(q.take((void**)&tabs, sizeof(RowTab) * nr));
  CJS_TRY(q.take((void**)&sel, (size_t)MAX_SELECTORS * nr));
  CJS_TRY(q.take((void**)&gstart, 4 * (size_t)(MAX_SELECTORS + 1) * nr));
  CJS_TRY(q.take((void**)&syms, 2 * (size_t)L.sym_groups * GROUP_SYMS * nr));
  if (!L.single) CJS_TRY(q.take((void**)&gdst, sizeof(RowDst) * nr));
  if (group) CJS_TRY(q.take((void**)&rlim, 4 * nr));
  if (L.single) S.d_tt = ttb;
  gdst_host.resize(L.single ? 0 : nr);
  return 0;
}

// Stage 2 of the batch's candidates (Huffman chain per block, the groups' symbols, (rank, offset) ops), single-stream or batch form,
// and their BlockOut records with the stream drained
static int decode_rows(ARun& a, const RowBatch& b) {
  DecShare& S = a.S; const RowLayout& L = a.L; const RowScratch& R = a.R;
  hipStream_t s = a.s;
  const uint32_t c0 = b.c0, nc = b.c1 - b.c0, rows = b.rows, r0 = b.r0, dsz = a.J.tt_stride;
  if (a.nin) launch_block_decode_batch(s, S.d_in, a.d_cend + c0, a.d_cend + a.ncand + c0, R.rlim, a.d_cand + c0, nc, rows, dsz, R.tabs, R.sel, R.gstart, R.l0, R.bo + c0, r0, L.group_tiles, R.syms,
                                       L.sym_stride, L.sym_groups, R.ops, R.opoff, L.ops_stride, R.nops);
  else {
    hipLaunchKernelGGL(bz_chain, dim3(nc), dim3(CH_T), 0, s, S.d_in, S.up_hi, a.d_cand + c0, nc, dsz, R.tabs, R.sel, R.gstart, R.l0, R.bo + c0, r0);
    if (rows) hipLaunchKernelGGL(bz_group_syms, dim3(L.group_tiles, rows), dim3(256), 0, s, S.d_in, S.up_hi, R.tabs, R.sel, R.gstart, R.syms, L.sym_stride, L.sym_groups, 0u);
    hipLaunchKernelGGL(bz_sym_ops, dim3(nc), dim3(1024), 0, s, R.tabs, a.d_cand + c0, nc, R.syms, L.sym_groups, dsz, R.ops, R.opoff, L.ops_stride, R.nops, R.bo + c0, r0, S.up_hi * 8);
  }
  DEC_HIP(hipGetLastError());
  DEC_HIP(hipMemcpyAsync(S.bos.data() + c0, R.bo + c0, sizeof(BlockOut) * nc, hipMemcpyDeviceToHost, s));
  DEC_HIP(hipStreamSynchronize(s));
  S.d2h += sizeof(BlockOut) * (size_t)nc;
  return 0;
}
// Move-to-front of the batch's rows: all 256-op tiles in parallel, the tiles' start lists chained, emit
static int mtf_rows(ARun& a, const RowBatch& b) {
  const DecShare& S = a.S; const RowLayout& L = a.L; const RowScratch& R = a.R;
  hipStream_t s = a.s;
  const uint32_t rows = b.rows;
  uint32_t maxc = 0;
  for (uint32_t c = b.c0; c < b.c1; c++) if (S.cands[c].kind == 0 && !S.bos[c].err) maxc = std::max(maxc, S.bos[c].count);
  const uint32_t tiles_used = std::min<uint32_t>(maxc / MT_TILE + 1u, L.tiles_per_row);
  // slabs of rows: grid.y <= 65535 and grid.x * grid.y * 256 threads < 2^32 (a larger launch is cut short without an error)
  const uint32_t slab = std::min<uint32_t>(65535u, std::max<uint32_t>(1u, (1u << 23) / tiles_used));
  for (uint32_t q0 = 0; q0 < rows; q0 += slab)
    hipLaunchKernelGGL(bz_mtf_tiles, dim3((tiles_used + 3u) / 4u, std::min(slab, rows - q0)), dim3(256), 0, s, R.ops, L.ops_stride, R.nops, R.pl, L.tiles_per_row, q0);
  const uint32_t chunks = (tiles_used + MC_TILES - 1) / MC_TILES;       // (the symbols are spent: their rows hold the chunks' products)
  const size_t cstride = 2 * (size_t)L.sym_groups * GROUP_SYMS;
  hipLaunchKernelGGL(bz_mtf_chunk_perm, dim3(chunks, rows), dim3(256), 0, s, R.nops, R.pl, L.tiles_per_row, reinterpret_cast<uint8_t*>(R.syms), cstride);
  hipLaunchKernelGGL(bz_mtf_compose, dim3(chunks, rows), dim3(256), 0, s, R.nops, R.l0, R.pl, L.tiles_per_row, reinterpret_cast<const uint8_t*>(R.syms), cstride);
  for (uint32_t q0 = 0; q0 < rows; q0 += slab)
    hipLaunchKernelGGL(bz_mtf_emit, dim3(tiles_used, std::min(slab, rows - q0)), dim3(256), 0, s, R.ops, R.opoff, L.ops_stride, R.nops, R.l0, R.pl, L.tiles_per_row, q0, R.ttb, a.J.tt_stride);
  DEC_HIP(hipGetLastError());
  return 0;
}
// one batch: the decoded rows stay where they are
static int keep_rows(ARun& a, const RowBatch& b) {
  DecShare& S = a.S;
  for (uint32_t c = b.c0; c < b.c1; c++) if (S.cands[c].kind == 0) S.tt_ptr[c] = (uint64_t)(uintptr_t)(a.R.ttb + (size_t)(S.cands[c].pad - b.r0) * a.J.tt_stride);
  return 0;
}
// several batches: the batch's decoded bytes packed into a buffer of their exact size (kept until the share is released)
static int pack_rows(ARun& a, const RowBatch& b) {
  DecShare& S = a.S; RowScratch& R = a.R;
  uint64_t packed = 0;
  for (uint32_t c = b.c0; c < b.c1; c++) if (S.cands[c].kind == 0 && !S.bos[c].err) packed += ((uint64_t)S.bos[c].count + 15u) & ~15ull;
  uint8_t* seg = nullptr;
  CJS_TRY(S.take((void**)&seg, (size_t)packed + 16));
  uint64_t at = 0;
  for (uint32_t c = b.c0; c < b.c1; c++) if (S.cands[c].kind == 0) {
    const uint32_t row = S.cands[c].pad - b.r0, cnt = S.bos[c].err ? 0u : S.bos[c].count;
    R.gdst_host[row] = RowDst{(uint64_t)(uintptr_t)(seg + at), cnt};
    S.tt_ptr[c] = (uint64_t)(uintptr_t)(seg + at);
    at += ((uint64_t)cnt + 15u) & ~15ull;
  }
  DEC_HIP(hipMemcpyAsync(R.gdst, R.gdst_host.data(), sizeof(RowDst) * (size_t)b.rows, hipMemcpyHostToDevice, a.s));
  S.h2d += sizeof(RowDst) * (size_t)b.rows;
  hipLaunchKernelGGL(bz_rows_pack, dim3(16, b.rows), dim3(256), 0, a.s, R.ttb, a.J.tt_stride, R.gdst);
  DEC_HIP(hipGetLastError());
  return 0;
}
static void debug_lines(ARun& a) {
  DecShare& S = a.S;
  uint64_t clk[8];
  if (!a.nin && hipMemcpyFromSymbol(clk, HIP_SYMBOL(g_dec_clk), sizeof clk) == hipSuccess) {
    S.d2h += sizeof clk;
    fprintf(stderr, "[cjs dec] candidate 0: header + tables %.1f us, group chain %.1f us for %llu groups\n", clk[5] / 100.0, clk[6] / 100.0, (unsigned long long)clk[7]);
  }
  fprintf(stderr, "[cjs dec] share on device %d: bytes [%llu, %llu) uploaded [%llu, %llu) = %zu B, %u candidates\n", S.device, (unsigned long long)S.lo,
          (unsigned long long)S.hi, (unsigned long long)S.up_lo, (unsigned long long)S.up_hi, a.up_n, a.ncand);
}

static int phase_a(DecJob& J, DecShare& S) {
  ARun a{J, S, S.s, ShareScratch(&S), (size_t)(S.up_hi - S.up_lo), (uint32_t)S.bst.size()};
  CJS_TRY(upload(a));
  CJS_TRY(candidates(a));
  const uint64_t cut = row_limit_trim(S.cands, S.row_from, S.row_limit);      // (a streaming step: see DecShare)
  if (cut != ~0ull) S.cut_bit = cut;
  a.ncand = (uint32_t)S.cands.size();
  CJS_TRY(number_rows(a));
  if (!a.ncand) return 0;
  // Block decode in three stages (Huffman chain per block -> (rank, offset) ops; move-to-front of all 256-op tiles in parallel;
  // emit), over BATCHES of rows: a row of scratch is sized for a whole block of the file's largest level (~7 x tt_stride bytes),
  // whatever the candidate turns out to hold, so a file of very many tiny member streams (or one stuffed with block magics)
  // must not get a row per candidate at once.  One batch (the usual case: <= ~2000 level-9 rows in 16 GiB: a 2^30-byte stream has 1,194) keeps its decoded
  // rows where they are; with several batches each batch's decoded bytes are packed into a buffer of their exact size and
  // the scratch rows are used again.
  static const uint64_t budget = getenv("CJS_DEC_ROW_BYTES") ? strtoull(getenv("CJS_DEC_ROW_BYTES"), nullptr, 10) : (16ull << 30);      // (tests shrink it)
  a.L = row_layout(J.tt_stride, a.nrows, budget, MT_TILE, sizeof(RowTab));
  CJS_TRY(a.R.take(S, a.q, a.L, J.tt_stride, a.ncand, a.nin != 0));
  for (uint32_t c0 = 0; c0 < a.ncand;) {
    const RowBatch b = row_batch(S.cands.data(), a.ncand, c0, a.L.nr);
    S.a_batches++;
    CJS_TRY(decode_rows(a, b));
    if (b.rows) {
      CJS_TRY(mtf_rows(a, b));
      CJS_TRY(a.L.single ? keep_rows(a, b) : pack_rows(a, b));
      DEC_HIP(hipStreamSynchronize(a.s));
    }
    c0 = b.c1;
  }
  if (env_debug()) debug_lines(a);
  a.q.done();                                                           // (every batch ended with the stream drained)
  return 0;
}
void dec_phase_a(DecJob* J, DecShare* S) {
  const auto T0 = std::chrono::steady_clock::now();
  const bool ready = hipSetDevice(S->device) == hipSuccess && (S->s || hipStreamCreate(S->s.put()) == hipSuccess);      // (a device source made the stream for the header pass)
  S->rc = ready ? phase_a(*J, *S) : (int)CJS_E_HIP;
  S->ms_a = ms_since(T0);
}

}  // namespace cjs
