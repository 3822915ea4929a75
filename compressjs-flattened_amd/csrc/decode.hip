// decode.hip — Bzip2.decompressFile (Bunzip.decode, J/Bzip2_joined_.js:1769-1796) on the MI355X.
//
// The reference decodes block after block from one bit cursor.  Blocks carry no length field, so here:
//   1. bz_magic_scan     every bit offset of the stream is tested against the 48-bit block / end-of-stream
//                        magics (:1434-1439) -> candidate list (a few hundred entries);
//   2. bz_decode_block   one wave per candidate: header, selector list, code-length tables, then the
//                        bit-serial Huffman + RUNA/RUNB + MTF decode (:1456-1670) on lane 0 with
//                        10-bit direct lookup tables built by the whole wave from the reference's
//                        limit/base/permute semantics; yields the BWT bytes, their histogram, the end bit;
//   3. host              walks the chain 32 -> end(block0) -> end(block1) ... over the candidates (a false
//                        2^-48 candidate inside payload bits is simply never reached), folds CRCs;
//   4. inverse BWT       T vector by a stable radix pass keyed (block, byte) (:1677-1690), then the LF walk
//                        (:1732-1737) — n dependent gathers — made k-way parallel by splitter list ranking:
//                        every 128th slot is a splitter, lanes walk to the next splitter, one workgroup per block
//                        ranks the splitters (pointer jumping in LDS), lanes re-walk writing bytes at their final offsets;
//   5. RLE1 expansion    (:1738-1753) parsed in parallel: a count byte follows 4 equal literals; inside a
//                        stretch of equal bytes the literal/count phase has period 5 and the only carried
//                        state (does the stretch start with a count byte?) is a 2-state function scan;
//   6. CRC check         per block over the output bytes (rle1.hip's slice + GF(2) combine), :1756-1761.
// Recovery of damaged data (cjs_bzip2_recover, no reference equivalent: the job of bzip2recover) is 1, 2 and 4-6 over EVERY
// decodable candidate, with step 3 replaced by a selection of the intact, non-overlapping ones; its repaired-stream form gathers
// their bit strings into a new stream (bz_bits_gather).
#include "cjs_internal.h"
#include "bz_index.h"
#include "host.h"
#include "prims.hpp"
#include "rle1.h"
#include <algorithm>
#include <chrono>
#include <functional>
#include <memory>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using namespace cjs;

#include "decode_dev.h"

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

// ---------------------------------------------------------------- 4. inverse BWT
struct IbBlock {            // per valid block, in stream order
  uint64_t tt;              // device address of the block's decoded BWT bytes
  uint32_t count;           // n
  uint32_t orig;
  uint32_t off;             // element offset of the block in the concatenated sort / LF arrays
  uint32_t woff;            // byte offset of the block in the walk's output (w)
  uint64_t out_off;         // byte offset of the block in the final output
  uint32_t out_len;
  uint32_t crc;
};

// keys (block << 8 | byte), vals = i
__global__ __launch_bounds__(256) void ib_make_keys(const IbBlock* __restrict__ blocks, uint32_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t stride) {
  const IbBlock b = blocks[blockIdx.y];
  const uint8_t* __restrict__ tt = reinterpret_cast<const uint8_t*>(b.tt);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < b.count; i += gridDim.x * 256) {
    key[b.off + i] = ((uint32_t)blockIdx.y << 8) | tt[i];
    val[b.off + i] = i;
  }
}
// For the segmented pass every block owns `stride` slots (one segment each), and a key is (i << 8) | byte -- the index rides on the
// key, there is no value array (a block has < 2^24 bytes); the slots behind the block's bytes hold the largest digit, which the stable
// sort leaves behind everything real.  One workgroup per radix tile (RS_TILE slots of a block's range): the keys, and the tile's count of
// every byte -- the row of the histogram the pass would otherwise read the keys again for (four copies per wave, interleaved: see
// rs_hist_bytes)
__global__ __launch_bounds__(256) void ib_make_keys_hist(const IbBlock* __restrict__ blocks, uint32_t* __restrict__ key, uint32_t stride, uint32_t tps,
                                                         uint32_t* __restrict__ hist) {
  constexpr int HC = 4;
  __shared__ uint32_t h[4 * 256 * HC];
  const IbBlock b = blocks[blockIdx.y];
  const uint8_t* __restrict__ tt = reinterpret_cast<const uint8_t*>(b.tt);
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4 * HC; i++) h[i * 256 + tid] = 0;
  __syncthreads();
  uint32_t* hw = h + (tid >> 6) * 256 * HC + (tid & (HC - 1));
  const uint32_t t0 = blockIdx.x * RS_TILE;
#pragma unroll 4
  for (uint32_t e = tid; e < RS_TILE; e += 256) {
    const uint32_t i = t0 + e;
    if (i < stride) {
      const uint32_t by = i < b.count ? tt[i] : 0xFFu;
      key[b.off + i] = i < b.count ? (i << 8) | by : 0xFFu;
      atomicAdd(&hw[by * HC], 1u);
    }
  }
  __syncthreads();
  uint32_t sum = 0;
#pragma unroll
  for (int w = 0; w < 4; w++)
#pragma unroll
    for (int r = 0; r < HC; r++) sum += h[w * 256 * HC + tid * HC + r];
  hist[((size_t)blockIdx.y * tps + blockIdx.x) * 256 + tid] = sum;
}
// after the stable sort: slot j of the block holds (T[j] << 8) | tt[j] == the reference's dbuf (:1686-1690):
// the pointer comes from the sorted order, the low byte is the j-th DECODED byte (not the sorted one)
// (on_key: the sorted array holds (i << 8) | sorted byte, see ib_make_keys)
__global__ __launch_bounds__(256) void ib_pack(const IbBlock* __restrict__ blocks, const uint32_t* __restrict__ val, uint32_t* __restrict__ dbuf, int on_key) {
  const IbBlock b = blocks[blockIdx.y];
  const uint8_t* __restrict__ tt = reinterpret_cast<const uint8_t*>(b.tt);
  for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < b.count; j += gridDim.x * 256)
    dbuf[b.off + j] = (on_key ? val[b.off + j] & 0xFFFFFF00u : val[b.off + j] << 8) | tt[j];
}
// sentinel variant (BWT.unbwtransform, J/BWTC_joined_.js:1147-1168): next(t) = LF[t] + C[T[t]] (+1 below pidx) = the stable
// sorted position of element t; slot t holds (next(t) << 8) | T[t].  b.orig carries pidx.
__global__ __launch_bounds__(256) void ib_pack_sentinel(const IbBlock* __restrict__ blocks, const uint32_t* __restrict__ val, uint32_t* __restrict__ dbuf) {
  const IbBlock b = blocks[blockIdx.y];
  const uint8_t* __restrict__ tt = reinterpret_cast<const uint8_t*>(b.tt);
  for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < b.count; j += gridDim.x * 256) {
    const uint32_t t = val[b.off + j];
    dbuf[b.off + t] = ((j + (j < b.orig ? 1u : 0u)) << 8) | tt[t];
  }
}
// splitters: slot j with j % SPL == 0, plus the start slot.  Walk until the next splitter.
__device__ __forceinline__ bool is_split(uint32_t j, uint32_t start) { return (j % SPL) == 0 || j == start; }
// The walks below are n dependent random 4-byte reads per block.  With every block's walkers spread over the chip each XCD's
// 4 MiB L2 sees all blocks' vectors (3.6 MB each at level 9) and every step is a 64-byte fetch from memory: 2.4 + 3.2 ms per
// 100 MB.  So (1) workgroup 8 j + x -- it runs on XCD x -- takes chunk x * ceil(T / 8) + j of the (block, 256 splitters) chunks:
// an XCD works through a contiguous range of blocks; (2) the launches ask for WALK_LDS bytes of LDS they never touch, which
// leaves five workgroups per CU: 40 K walkers per XCD, the splitters of about six blocks.  Measured (walk1 + walk2 per 100 MB):
// blocks spread over the chip 5.57 ms; XCD ranges with 0 / 30 / 60 / 100 KB of LDS asked for 4.71 / 4.06 / 4.11 / 5.51 ms -- fewer
// blocks in flight hit the L2 more often but leave too few walkers to hide what still misses (with a splitter every 64 slots:
// 0 / 16 / 30 / 45 / 60 KB 3.53 / 3.51 / 2.90 / 2.91 / 3.32 ms).
constexpr uint32_t WALK_T = 256, WALK_LDS = 30 * 1024;
__host__ __device__ __forceinline__ uint32_t walk_chunks(uint32_t max_count) { return ((max_count + SPL - 1) / SPL + 1 + WALK_T - 1) / WALK_T; }
__device__ __forceinline__ bool walk_item(uint32_t nblocks, uint32_t cpb, uint32_t& blk, uint32_t& sidx) {
  const uint32_t T = nblocks * cpb, per = (T + 7u) >> 3;
  const uint32_t t = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
  if (t >= T) return false;
  blk = t / cpb; sidx = (t - blk * cpb) * WALK_T + threadIdx.x;
  return true;
}
constexpr uint32_t SPL_END = 0xFFFFFFFEu;   // the chain left the block (sentinel variant: the row of the implicit end marker)
// `seg` (cyclic form): the walk also KEEPS what it reads -- the bytes of the first SEG_CAP slots it visits, SEG_CAP bytes per splitter,
// sixteen at a time -- and the slot it stands on after SEG_CAP steps (`resume`): once the splitters are ranked the bytes only have
// to be put in their places (ib_place), and a second walk (ib_walk2) is left for what the few long stretches hold behind SEG_CAP.
// (Both walks were the same 100 M random 4-byte reads, a 64-byte line each: about 1.1 ms per 100 MB apiece.)
constexpr uint32_t SEG_CAP = 384;           // a stretch is longer with probability e^-6
__global__ __launch_bounds__(WALK_T) void ib_walk1(const uint32_t* __restrict__ dbuf, const IbBlock* __restrict__ blocks, uint32_t nblocks, uint32_t cpb,
                                                   uint32_t spl_stride, uint32_t* __restrict__ spl_next, uint32_t* __restrict__ spl_steps, int sentinel,
                                                   uint8_t* __restrict__ seg, uint32_t* __restrict__ resume) {
  uint32_t blk, sidx;
  if (!walk_item(nblocks, cpb, blk, sidx)) return;
  const IbBlock b = blocks[blk];
  const uint32_t* d = dbuf + b.off;
  const uint32_t nspl = (b.count + SPL - 1) / SPL + 1;         // regular splitters + one slot for `start`
  if (sidx >= nspl) return;
  const uint32_t start = sentinel ? 0u : d[b.orig] >> 8;       // first slot visited by the loop (:1698-1700)
  uint32_t pos;
  if (sidx == nspl - 1) { pos = start; if ((start % SPL) == 0) { spl_steps[(size_t)blk * spl_stride + sidx] = 0; spl_next[(size_t)blk * spl_stride + sidx] = start / SPL; return; } }
  else pos = sidx * SPL;
  uint32_t steps = 0, cur = pos;
  if (seg) {
    uint4* sb = reinterpret_cast<uint4*>(seg + ((size_t)blk * spl_stride + sidx) * SEG_CAP);
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    do {
      const uint32_t e = d[cur];
      if (steps < SEG_CAP) {
        const uint32_t k = (steps >> 2) & 3u;
#pragma unroll
        for (int t = 0; t < 4; t++) if (k == (uint32_t)t) acc[t] = (acc[t] >> 8) | (e << 24);
        if ((steps & 15u) == 15u) sb[steps >> 4] = make_uint4(acc[0], acc[1], acc[2], acc[3]);
      }
      cur = e >> 8; steps++;
      if (steps == SEG_CAP) resume[(size_t)blk * spl_stride + sidx] = cur;
    } while (cur < b.count && !is_split(cur, start) && steps < b.count);
    if (steps < SEG_CAP && (steps & 15u)) {                    // the open piece: its words' bytes stand at the top
      const uint32_t k = (steps >> 2) & 3u, r = 8u * (4u - (steps & 3u));
#pragma unroll
      for (int t = 0; t < 4; t++) if (k == (uint32_t)t && (steps & 3u)) acc[t] >>= r;
      sb[steps >> 4] = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    }
  } else {
    do { cur = d[cur] >> 8; steps++; } while (cur < b.count && !is_split(cur, start) && steps < b.count);
  }
  spl_steps[(size_t)blk * spl_stride + sidx] = steps;
  spl_next[(size_t)blk * spl_stride + sidx] = cur >= b.count ? SPL_END : (cur == start && (start % SPL) != 0) ? nspl - 1 : cur / SPL;
}
// the kept bytes of 64 stretches (splitters s0 .. s0 + 63 of block b, their ranks and lengths one per lane) to their places: four
// stretches in flight at a time, the lanes along the bytes
__device__ __forceinline__ void ib_place64(const IbBlock& b, size_t at0, uint32_t s0, uint32_t nspl, const uint32_t* __restrict__ spl_rank,
                                           const uint32_t* __restrict__ spl_steps, const uint8_t* __restrict__ seg, uint8_t* __restrict__ w) {
  const int lane = lane_id();
  uint32_t rank = 0, nbytes = 0;
  if (s0 + lane < nspl) {
    rank = spl_rank[at0 + lane];
    const uint32_t steps = spl_steps[at0 + lane];
    if (rank != 0xFFFFFFFFu && steps != 0 && rank < b.count) nbytes = min(min(steps, SEG_CAP), b.count - rank);
  }
  const uint8_t* src = seg + at0 * SEG_CAP;
  for (int i = 0; i < 64; i += 4) {
    uint32_t r[4], nb[4], mx = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { r[j] = (uint32_t)__builtin_amdgcn_readlane((int)rank, i + j); nb[j] = (uint32_t)__builtin_amdgcn_readlane((int)nbytes, i + j); mx = max(mx, nb[j]); }
    for (uint32_t o = lane; o < mx; o += 64) {
      uint8_t v[4];
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = o < nb[j] ? src[(size_t)(i + j) * SEG_CAP + o] : (uint8_t)0;
#pragma unroll
      for (int j = 0; j < 4; j++) if (o < nb[j]) w[r[j] + o] = v[j];
    }
  }
}
__global__ __launch_bounds__(256) void ib_place(const IbBlock* __restrict__ blocks, uint32_t spl_stride, const uint32_t* __restrict__ spl_rank,
                                                const uint32_t* __restrict__ spl_steps, const uint8_t* __restrict__ seg, uint8_t* __restrict__ wbuf) {
  const IbBlock b = blocks[blockIdx.y];
  const uint32_t nspl = (b.count + SPL - 1) / SPL + 1, s0 = (blockIdx.x * 4u + (uint32_t)wave_id()) * 64u;
  if (s0 < nspl) ib_place64(b, (size_t)blockIdx.y * spl_stride + s0, s0, nspl, spl_rank, spl_steps, seg, wbuf + b.woff);
}
// rank the splitter chain from `start`: spl_rank[s] = number of output positions before splitter s's segment.
// One workgroup per block.  The chain is a list of <= 14064 nodes (a cycle through the start node for a cyclic BWT): the
// edge back into the first node is cut and the suffix sums of the segment lengths come from pointer jumping in LDS
// (14 rounds) instead of 14000 dependent loads; rank = total - suffix sum.  If the total is not the block length the
// permutation has a short cycle (periodic block) and lane 0 walks the chain the slow way, as the reference would.
constexpr uint32_t IBR_MAX = 14080;      // >= 900000 / SPL + 2
constexpr int IBR_PT = (IBR_MAX + 1023) / 1024;      // nodes per thread
__global__ __launch_bounds__(1024) void ib_rank(const IbBlock* __restrict__ blocks, uint32_t nblocks, uint32_t spl_stride, const uint32_t* __restrict__ spl_next,
                                                const uint32_t* __restrict__ spl_steps, uint32_t* __restrict__ spl_rank, int32_t* __restrict__ err) {
  __shared__ uint32_t nxt[IBR_MAX], dst[IBR_MAX];
  __shared__ uint32_t s_total;
  const uint32_t k = blockIdx.x;
  if (k >= nblocks) return;
  const IbBlock b = blocks[k];
  const uint32_t nspl = (b.count + SPL - 1) / SPL + 1;
  const uint32_t* nx = spl_next + (size_t)k * spl_stride; const uint32_t* st = spl_steps + (size_t)k * spl_stride;
  uint32_t* rk = spl_rank + (size_t)k * spl_stride;
  bool fast = nspl <= IBR_MAX;
  if (fast) {
    const uint32_t entry = nspl - 1;
    const bool alias = st[entry] == 0;                 // start % SPL == 0: the start entry only points at the regular splitter
    const uint32_t head = alias ? nx[entry] : entry;
    for (uint32_t i = threadIdx.x; i < nspl; i += 1024) {
      uint32_t n = nx[i];
      if (n == head && !(alias && i == entry)) n = SPL_END;       // the edge that closes the cycle
      if (n != SPL_END && n >= nspl) n = SPL_END;
      nxt[i] = n; dst[i] = st[i];
    }
    __syncthreads();
    for (uint32_t span = 1; span < nspl; span <<= 1) {
      uint32_t nn[IBR_PT], dd[IBR_PT];
#pragma unroll
      for (int q = 0; q < IBR_PT; q++) {
        const uint32_t i = threadIdx.x + 1024u * q;
        nn[q] = SPL_END; dd[q] = 0;
        if (i < nspl) { const uint32_t n = nxt[i]; if (n != SPL_END) { nn[q] = nxt[n]; dd[q] = dst[n]; } else nn[q] = SPL_END; }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < IBR_PT; q++) {
        const uint32_t i = threadIdx.x + 1024u * q;
        if (i < nspl && nxt[i] != SPL_END) { dst[i] += dd[q]; nxt[i] = nn[q]; }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) s_total = dst[entry];
    __syncthreads();
    const uint32_t total = s_total;
    if (total == b.count) {
      for (uint32_t i = threadIdx.x; i < nspl; i += 1024) rk[i] = total - dst[i];
      if (threadIdx.x == 0) err[k] = (int32_t)total;
      return;
    }
    fast = false;
  }
  if (threadIdx.x != 0) return;
  for (uint32_t i = 0; i < nspl; i++) rk[i] = 0xFFFFFFFFu;
  uint32_t cur = nspl - 1, done = 0;
  // the start splitter may alias a regular one (start % SPL == 0): its entry has steps 0 and points at it
  for (uint32_t guard = 0; guard <= nspl + 1 && done < b.count; guard++) {
    if (rk[cur] != 0xFFFFFFFFu && st[cur] != 0) break;           // back on a visited splitter: the permutation has a short cycle
    rk[cur] = done; done += st[cur]; cur = nx[cur];
    if (cur == SPL_END) break;
  }
  // done < count: the LF permutation has a short cycle (periodic block, e.g. "abab"): the reference keeps walking
  // round it for `count` steps (:1732), i.e. the byte sequence is periodic with period `done`
  err[k] = (int32_t)done;
}
__global__ __launch_bounds__(256) void ib_periodic_fill(const IbBlock* __restrict__ blocks, const int32_t* __restrict__ cyc, uint8_t* __restrict__ wbuf) {
  const IbBlock b = blocks[blockIdx.y];
  const uint32_t L = (uint32_t)cyc[blockIdx.y];
  if (L == 0 || L >= b.count) return;
  uint8_t* w = wbuf + b.woff;
  for (uint32_t r = L + blockIdx.x * 256 + threadIdx.x; r < b.count; r += gridDim.x * 256) w[r] = w[r % L];
}
// second walk: write the pre-RLE1 byte sequence w[0..n) of each block (w[r] = byte of the (r+1)-th visited slot)
__global__ __launch_bounds__(WALK_T) void ib_walk2(const uint32_t* __restrict__ dbuf, const IbBlock* __restrict__ blocks, uint32_t nblocks, uint32_t cpb,
                                                   uint32_t spl_stride, const uint32_t* __restrict__ spl_rank, const uint32_t* __restrict__ spl_steps,
                                                   uint8_t* __restrict__ wbuf, int sentinel, const uint32_t* __restrict__ resume, const uint8_t* __restrict__ seg) {
  uint32_t blk, sidx;
  if (!walk_item(nblocks, cpb, blk, sidx)) return;
  const IbBlock b = blocks[blk];
  const uint32_t* d = dbuf + b.off;
  uint8_t* w = wbuf + b.woff;
  const uint32_t nspl = (b.count + SPL - 1) / SPL + 1;
  if (sidx >= nspl) return;
  const uint32_t start = sentinel ? 0u : d[b.orig] >> 8;
  uint32_t rank = spl_rank[(size_t)blk * spl_stride + sidx], steps = spl_steps[(size_t)blk * spl_stride + sidx];
  if (rank == 0xFFFFFFFFu || steps == 0) return;
  uint32_t cur = sidx == nspl - 1 ? start : sidx * SPL;
  if (seg) {                                      // only what ib_walk1 did not keep: from the slot it stood on after SEG_CAP steps
    if (steps <= SEG_CAP) return;
    cur = resume[(size_t)blk * spl_stride + sidx]; rank += SEG_CAP; steps -= SEG_CAP;
    if (rank >= b.count) return;
  }
  // visiting order: position `rank` of the walk is slot `cur`; the loop outputs the byte of every visited slot (:1735-1736)
  if (sentinel) {
    for (uint32_t q = 0; q < steps && rank + q < b.count; q++) {
      const uint32_t e = d[cur];
      w[b.count - 1 - (rank + q)] = (uint8_t)(e & 0xFF);                         // unbwtransform fills U from the end (BWTC:1161)
      cur = e >> 8;
    }
    return;
  }
  // A lane's bytes are neighbours in w, the lanes' stretches are not: a byte per store is 64 lines per wave instruction, and the
  // stores, not the reads, set the pace.  Whole aligned 16-byte pieces of the stretch go out as such, the words and then the bytes in
  // front of the first and behind the last one by one (they share their pieces with the stretches of other lanes).
  const uint32_t r1 = min(rank + steps, b.count);
  uint32_t r = rank;
  auto word = [&]() { uint32_t acc = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) { const uint32_t e = d[cur]; acc = (acc >> 8) | (e << 24); cur = e >> 8; }
    return acc; };
  for (; r < r1 && ((b.woff + r) & 3u); r++) { const uint32_t e = d[cur]; w[r] = (uint8_t)e; cur = e >> 8; }
  for (; r + 4 <= r1 && ((b.woff + r) & 15u); r += 4) *reinterpret_cast<uint32_t*>(w + r) = word();
  for (; r + 16 <= r1; r += 16) { uint4 q; q.x = word(); q.y = word(); q.z = word(); q.w = word(); *reinterpret_cast<uint4*>(w + r) = q; }
  for (; r + 4 <= r1; r += 4) *reinterpret_cast<uint32_t*>(w + r) = word();
  for (; r < r1; r++) { const uint32_t e = d[cur]; w[r] = (uint8_t)e; cur = e >> 8; }
}

// ---------------------------------------------------------------- 5. RLE1 expansion
// Stretch functions on the carried bit c0 ("this stretch starts with a count byte"): next = ((L - c0) % 5 == 4)
//   L % 5 == 4 -> NOT-ish (c0=0 ->1, c0=1 -> 0), L % 5 == 0 -> identity, else const 0.  Encoded as 2 bits (f(0) | f(1) << 1).
__device__ __forceinline__ uint32_t stretch_fn(uint32_t L) { const uint32_t m = L % 5; return m == 4 ? 1u : (m == 0 ? 2u : 0u); }
__device__ __forceinline__ uint32_t fn_apply(uint32_t f, uint32_t c) { return (f >> c) & 1u; }
__device__ __forceinline__ uint32_t fn_compose(uint32_t first, uint32_t then) {     // x -> then(first(x))
  return fn_apply(then, fn_apply(first, 0)) | (fn_apply(then, fn_apply(first, 1)) << 1);
}
// One tile (UR_TILE = 1024 threads x UR_BPT bytes) of a block by one workgroup.  Carried from the tiles in front: start of the current stretch,
// c0 of the current stretch, output bytes so far (from the length pass below); the bytes go out.
constexpr int UR_BPT_C = 16;
// A thread's UR_BPT = 16 bytes w[p0 .. p0 + 16) and the byte in front of them (0 at the block's first byte), bytes behind the block's
// end as 0.  The address has any alignment (the same for the whole workgroup): two aligned 16-byte loads and a funnel shift (a byte
// per load was 17 instructions of 16 lines each; the walk's output buffer has 64 bytes of slack behind its last block).
__device__ __forceinline__ void ur_load(const uint8_t* __restrict__ w, uint32_t n, uint32_t p0, uint8_t (&c)[UR_BPT_C + 1]) {
  const uintptr_t A = (uintptr_t)(w + p0);
  const uint4* q = reinterpret_cast<const uint4*>(A & ~(uintptr_t)15);
  const uint32_t r = 8u * ((uint32_t)A & 3u);
  uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
  if (p0 < n) { lo = q[0]; hi = q[1]; }             // (at most 31 bytes behind the block's end)
  uint32_t d[4];
  switch (((uint32_t)A >> 2) & 3u) {              // (uniform)
    case 0: d[0] = __funnelshift_r(lo.x, lo.y, r); d[1] = __funnelshift_r(lo.y, lo.z, r); d[2] = __funnelshift_r(lo.z, lo.w, r); d[3] = __funnelshift_r(lo.w, hi.x, r); break;
    case 1: d[0] = __funnelshift_r(lo.y, lo.z, r); d[1] = __funnelshift_r(lo.z, lo.w, r); d[2] = __funnelshift_r(lo.w, hi.x, r); d[3] = __funnelshift_r(hi.x, hi.y, r); break;
    case 2: d[0] = __funnelshift_r(lo.z, lo.w, r); d[1] = __funnelshift_r(lo.w, hi.x, r); d[2] = __funnelshift_r(hi.x, hi.y, r); d[3] = __funnelshift_r(hi.y, hi.z, r); break;
    default: d[0] = __funnelshift_r(lo.w, hi.x, r); d[1] = __funnelshift_r(hi.x, hi.y, r); d[2] = __funnelshift_r(hi.y, hi.z, r); d[3] = __funnelshift_r(hi.z, hi.w, r); break;
  }
#pragma unroll
  for (int j = 0; j < UR_BPT_C; j++) c[j + 1] = p0 + j < n ? (uint8_t)(d[j >> 2] >> (8 * (j & 3))) : (uint8_t)0;
  uint32_t prev = (uint32_t)__shfl_up((int)(d[3] >> 24), 1, 64);                 // the lane in front holds the byte in front (beyond n: never looked at)
  if (lane_id() == 0) prev = (p0 > 0 && p0 - 1 < n) ? w[p0 - 1] : 0u;
  c[0] = (uint8_t)prev;
}
struct RleCarry { uint32_t cur_start, cur_c0, out_base, pad; };
static_assert(UR_BPT_C == 16, "ur_load");
constexpr int UR_BPT = UR_BPT_C;                    // bytes per thread: the ten-step function scan over the 1024 threads is most of a tile, whatever the bytes per thread (4 bytes: 1.05 ms per 100 MB for the length pass)
constexpr uint32_t UR_TILE = 1024 * UR_BPT;
constexpr uint32_t UR_STAGE = 24 * 1024;      // bytes of a tile's output put together in LDS (a tile of plain text makes UR_TILE and a few)
template <bool WRITE>
__device__ __forceinline__ void unrle1_tile(const uint8_t* __restrict__ w, uint32_t n, uint32_t base, RleCarry& cy, uint8_t* __restrict__ o,
                                            uint32_t* sm, uint32_t* fnarr, uint32_t* posarr, uint8_t* stage) {
  const uint32_t p0 = base + threadIdx.x * UR_BPT;
  uint8_t c[UR_BPT + 1];
  ur_load(w, n, p0, c);
  // stretch boundaries inside my positions
  uint32_t bmask = 0, lastb = 0;
#pragma unroll
  for (int j = 0; j < UR_BPT; j++) { const uint32_t p = p0 + j; if (p < n && p > 0 && c[j + 1] != c[j]) { bmask |= 1u << j; lastb = p + 1; } }
  // previous boundary before my first position: max-scan of (boundary position + 1), 0 = none in this tile
  const uint32_t im = block_incl_max<1024>(lastb, sm);
  posarr[threadIdx.x] = im;
  __syncthreads();
  const uint32_t exb = threadIdx.x ? posarr[threadIdx.x - 1] : 0u;
  const uint32_t tile_last = posarr[1023];
  __syncthreads();
  // per-thread function = composition of the stretch functions of the boundaries in my positions (in order);
  // a boundary at p closes the stretch [prev_start, p) of length p - prev_start
  uint32_t f = 2u;   // identity
  {
    uint32_t ps = exb ? exb - 1 : cy.cur_start;
#pragma unroll
    for (int j = 0; j < UR_BPT; j++) if ((bmask >> j) & 1u) { const uint32_t p = p0 + j; f = fn_compose(f, stretch_fn(p - ps)); ps = p; }
  }
  // exclusive scan of function composition across the 1024 threads: shuffles inside the waves, the sixteen wave totals through LDS
  // (two barriers; as a ten-step Hillis-Steele scan in LDS, twenty barriers, this was most of a tile)
  uint32_t incl = f;
  {
    const int lane = lane_id(), wv = wave_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t other = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl = fn_compose(other, incl);           // (the earlier threads' function first)
    }
    if (lane == 63) fnarr[wv] = incl;
    __syncthreads();
    if (wv == 0) {
      uint32_t t = lane < 16 ? fnarr[lane] : 2u;
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) {
        const uint32_t other = (uint32_t)__shfl_up((int)t, d, 64);
        if (lane >= d) t = fn_compose(other, t);
      }
      if (lane < 16) fnarr[16 + lane] = t;                     // inclusive over the waves
    }
    __syncthreads();
  }
  const uint32_t wprefix = wave_id() ? fnarr[16 + wave_id() - 1] : 2u;          // all earlier waves
  uint32_t fex = (uint32_t)__shfl_up((int)incl, 1, 64);
  fex = lane_id() ? fn_compose(wprefix, fex) : wprefix;                          // composition of all earlier threads' functions
  const uint32_t fall = fnarr[16 + 15];
  __syncthreads();
  // c0 of the stretch governing my first position
  uint32_t c0 = fn_apply(fex, cy.cur_c0);
  uint32_t ps = exb ? exb - 1 : cy.cur_start;
  uint32_t cnt = 0, is_cnt = 0;
#pragma unroll
  for (int j = 0; j < UR_BPT; j++) {
    const uint32_t p = p0 + j;
    if (p < n) {
      if ((bmask >> j) & 1u) { c0 = fn_apply(stretch_fn(p - ps), c0); ps = p; }
      const uint32_t q = ps + c0;                             // first literal of the stretch
      const uint32_t rel = p >= q ? p - q : 0u;
      const uint32_t count_byte = ((p == ps) & c0) | ((p >= q) & ((rel % 5u) == 4u));
      is_cnt |= count_byte << j;
      cnt += count_byte ? (uint32_t)c[j + 1] : 1u;
    }
  }
  uint32_t tot;
  uint32_t off = cy.out_base + block_excl_sum<1024>(cnt, sm, tot);
  if (WRITE) {
    // The tile's bytes are one stretch of the output, a thread's a few of them at an odd address: they are put together in LDS (at the
    // stretch's own alignment) and leave as aligned 16-byte pieces; a tile of long runs that does not fit goes out byte by byte.
    uint8_t* dst = o + cy.out_base;
    const uint32_t al = (uint32_t)((uintptr_t)dst & 15u);
    const bool staged = tot <= UR_STAGE;
    uint32_t rel = off - cy.out_base;
    if (staged) {                                  // (uniform)
#pragma unroll
      for (int j = 0; j < UR_BPT; j++) {
        if (p0 + j < n) {
          if ((is_cnt >> j) & 1u) { const uint32_t k = c[j + 1]; const uint8_t v = c[j]; for (uint32_t q = 0; q < k; q++) stage[al + rel + q] = v; rel += k; }
          else stage[al + rel++] = c[j + 1];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < UR_BPT; j++) {
        if (p0 + j < n) {
          if ((is_cnt >> j) & 1u) { const uint32_t k = c[j + 1]; const uint8_t v = c[j]; for (uint32_t q = 0; q < k; q++) dst[rel + q] = v; rel += k; }
          else dst[rel++] = c[j + 1];
        }
      }
    }
    if (staged) {
      __syncthreads();
      const uint32_t lead = min((16u - al) & 15u, tot), body = (tot - lead) >> 4, tail = lead + (body << 4);
      if (threadIdx.x < lead) dst[threadIdx.x] = stage[al + threadIdx.x];
      for (uint32_t i = threadIdx.x; i < body; i += 1024) reinterpret_cast<uint4*>(dst + lead)[i] = reinterpret_cast<const uint4*>(stage + al + lead)[i];
      if (threadIdx.x < tot - tail) dst[tail + threadIdx.x] = stage[al + tail + threadIdx.x];
    }
  }
  cy.out_base += tot;
  if (tile_last) { cy.cur_c0 = fn_apply(fall, cy.cur_c0); cy.cur_start = tile_last - 1; }
}
// The length pass, every tile of every block at once, in three launches (one workgroup per block walking its tiles front to back took
// 0.63 ms per 100 MB).  A tile depends on what lies in front of it through three things only: where the stretch that runs into it
// started (the last boundary in front), the carried bit c0 of that stretch, and the bytes out so far.  So: (1) every tile's last
// boundary; (2) with the last boundary in front of it, every tile's function on c0 and its byte count for BOTH values of c0;
// (3) per block, one wave chains the functions and sums the counts: the state carried INTO every tile, for the write pass.
// The RleCarry slot of a tile holds the intermediate values: pad = last boundary + 1 (0: none), cur_c0 = function, cur_start /
// out_base = bytes for c0 = 0 / 1.
__global__ __launch_bounds__(1024) void unrle1_bounds(const uint8_t* __restrict__ wbuf, const IbBlock* __restrict__ blocks, RleCarry* __restrict__ carry, uint32_t tiles_per_block) {
  __shared__ uint32_t sm[16];
  const IbBlock b = blocks[blockIdx.y];
  const uint32_t base = blockIdx.x * UR_TILE;
  if (base >= b.count) return;
  const uint8_t* w = wbuf + b.woff;
  const uint32_t p0 = base + threadIdx.x * UR_BPT;
  uint8_t c[UR_BPT + 1];
  ur_load(w, b.count, p0, c);
  uint32_t lastb = 0;
#pragma unroll
  for (int j = 0; j < UR_BPT; j++) { const uint32_t p = p0 + j; if (p < b.count && p > 0 && c[j + 1] != c[j]) lastb = p + 1; }
  const uint32_t im = block_incl_max<1024>(lastb, sm);
  if (threadIdx.x == 1023) carry[(size_t)blockIdx.y * tiles_per_block + blockIdx.x].pad = im;
}
__global__ __launch_bounds__(1024) void unrle1_sums(const uint8_t* __restrict__ wbuf, const IbBlock* __restrict__ blocks, RleCarry* __restrict__ carry, uint32_t tiles_per_block) {
  __shared__ unsigned long long sm64[16];
  __shared__ uint32_t sm[16];
  __shared__ uint32_t fnarr[32];
  __shared__ uint32_t posarr[1024];
  __shared__ uint32_t s_start;
  const IbBlock b = blocks[blockIdx.y];
  const uint32_t base = blockIdx.x * UR_TILE, n = b.count;
  if (base >= n) return;
  const uint8_t* w = wbuf + b.woff;
  RleCarry* row = carry + (size_t)blockIdx.y * tiles_per_block;
  if (threadIdx.x == 0) {                         // the last boundary in front of the tile: as a rule in the tile in front
    uint32_t st = 0;
    for (uint32_t t = blockIdx.x; t-- > 0;) { const uint32_t lb = row[t].pad; if (lb) { st = lb - 1; break; } }
    s_start = st;
  }
  const uint32_t p0 = base + threadIdx.x * UR_BPT;
  uint8_t c[UR_BPT + 1];
  ur_load(w, n, p0, c);
  uint32_t bmask = 0, lastb = 0;
#pragma unroll
  for (int j = 0; j < UR_BPT; j++) { const uint32_t p = p0 + j; if (p < n && p > 0 && c[j + 1] != c[j]) { bmask |= 1u << j; lastb = p + 1; } }
  const uint32_t im = block_incl_max<1024>(lastb, sm);
  posarr[threadIdx.x] = im;
  __syncthreads();
  const uint32_t exb = threadIdx.x ? posarr[threadIdx.x - 1] : 0u;
  const uint32_t cur_start = s_start;
  uint32_t f = 2u;   // identity
  {
    uint32_t ps = exb ? exb - 1 : cur_start;
#pragma unroll
    for (int j = 0; j < UR_BPT; j++) if ((bmask >> j) & 1u) { const uint32_t p = p0 + j; f = fn_compose(f, stretch_fn(p - ps)); ps = p; }
  }
  uint32_t incl = f;
  {
    const int lane = lane_id(), wv = wave_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t other = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl = fn_compose(other, incl);
    }
    if (lane == 63) fnarr[wv] = incl;
    __syncthreads();
    if (wv == 0) {
      uint32_t t = lane < 16 ? fnarr[lane] : 2u;
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) {
        const uint32_t other = (uint32_t)__shfl_up((int)t, d, 64);
        if (lane >= d) t = fn_compose(other, t);
      }
      if (lane < 16) fnarr[16 + lane] = t;
    }
    __syncthreads();
  }
  const uint32_t wprefix = wave_id() ? fnarr[16 + wave_id() - 1] : 2u;
  uint32_t fex = (uint32_t)__shfl_up((int)incl, 1, 64);
  fex = lane_id() ? fn_compose(wprefix, fex) : wprefix;
  const uint32_t fall = fnarr[16 + 15];
  unsigned long long both = 0;                    // bytes out of my positions for c0 = 0 (low half) and c0 = 1 (high half) at the tile's start
#pragma unroll
  for (int v = 0; v < 2; v++) {
    uint32_t c0 = fn_apply(fex, (uint32_t)v), ps = exb ? exb - 1 : cur_start, cnt = 0;
#pragma unroll
    for (int j = 0; j < UR_BPT; j++) {
      const uint32_t p = p0 + j;
      if (p < n) {
        if ((bmask >> j) & 1u) { c0 = fn_apply(stretch_fn(p - ps), c0); ps = p; }
        const uint32_t q = ps + c0;
        const uint32_t rel = p >= q ? p - q : 0u;
        const uint32_t count_byte = ((p == ps) & c0) | ((p >= q) & ((rel % 5u) == 4u));
        cnt += count_byte ? (uint32_t)c[j + 1] : 1u;
      }
    }
    both |= (unsigned long long)cnt << (32 * v);
  }
  unsigned long long tot;
  block_excl_sum<1024>(both, sm64, tot);
  if (threadIdx.x == 0) { RleCarry& e = row[blockIdx.x]; e.cur_c0 = fall; e.cur_start = (uint32_t)tot; e.out_base = (uint32_t)(tot >> 32); }
}
__global__ __launch_bounds__(64) void unrle1_carries(IbBlock* __restrict__ blocks, RleCarry* __restrict__ carry, uint32_t tiles_per_block) {
  const IbBlock b = blocks[blockIdx.x];
  RleCarry* row = carry + (size_t)blockIdx.x * tiles_per_block;
  const uint32_t nt = (b.count + UR_TILE - 1) / UR_TILE;
  const int lane = lane_id();
  uint32_t prevb = 0, c0 = 0, out = 0;            // last boundary + 1 / carried bit / bytes out in front of the chunk of 64 tiles
  for (uint32_t t0 = 0; t0 < nt; t0 += 64) {
    const uint32_t t = t0 + lane;
    RleCarry e{0u, 2u, 0u, 0u};                   // (behind the last tile: no bytes, the identity, no boundary)
    if (t < nt) e = row[t];
    const uint32_t im = wave_incl_max(e.pad);
    uint32_t exm = (uint32_t)__shfl_up((int)im, 1, 64); if (lane == 0) exm = 0;
    exm = exm > prevb ? exm : prevb;
    uint32_t incl = e.cur_c0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t other = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl = fn_compose(other, incl);
    }
    uint32_t fex = (uint32_t)__shfl_up((int)incl, 1, 64); if (lane == 0) fex = 2u;
    const uint32_t c0_in = fn_apply(fex, c0);
    const uint32_t bytes = c0_in ? e.out_base : e.cur_start;
    const uint32_t isum = wave_incl_sum(bytes);
    if (t < nt) row[t] = RleCarry{exm ? exm - 1 : 0u, c0_in, out + isum - bytes, 0u};
    const uint32_t last_m = (uint32_t)__builtin_amdgcn_readlane((int)im, 63);
    prevb = last_m > prevb ? last_m : prevb;
    c0 = fn_apply((uint32_t)__builtin_amdgcn_readlane((int)incl, 63), c0);
    out += (uint32_t)__builtin_amdgcn_readlane((int)isum, 63);
  }
  if (lane == 0) blocks[blockIdx.x].out_len = out;
}
// write pass: every tile of every block by itself
__global__ __launch_bounds__(1024) void unrle1_write(const uint8_t* __restrict__ wbuf, const IbBlock* __restrict__ blocks, const RleCarry* __restrict__ carry,
                                                     uint32_t tiles_per_block, uint8_t* __restrict__ out) {
  __shared__ uint32_t sm[16];
  __shared__ uint32_t fnarr[1024];
  __shared__ uint32_t posarr[1024];
  const IbBlock b = blocks[blockIdx.y];
  const uint32_t base = blockIdx.x * UR_TILE;
  if (base >= b.count) return;
  RleCarry cy = carry[(size_t)blockIdx.y * tiles_per_block + blockIdx.x];
  __shared__ __attribute__((aligned(16))) uint8_t stage[UR_STAGE + 16];
  unrle1_tile<true>(wbuf + b.woff, b.count, base, cy, out + b.out_off, sm, fnarr, posarr, stage);
}

__global__ void ib_make_crc_ranges(const IbBlock* __restrict__ blocks, uint32_t nblocks, RleBlock* __restrict__ ranges, uint32_t* __restrict__ nb_dev) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) *nb_dev = nblocks;
  if (k >= nblocks) return;
  RleBlock r; r.s = blocks[k].out_off; r.e = blocks[k].out_off + blocks[k].out_len; r.r_end = 0; r.Gr = 0; r.len = 0; r.base = 0;
  ranges[k] = r;
}

}  // namespace cjs

// ---------------------------------------------------------------- inverse sentinel BWT of a batch (used by BWTC.decompressFile)
namespace cjs {
// d_T holds the blocks back to back (block k at the sum of the earlier lengths), max_len bounds every block length.
// Blocks are processed in slabs of <= 65535 (grid.y of the per-block kernels) and <= 2^28 elements (bounded scratch).
static int ibwt_sentinel_slab(hipStream_t s, const uint8_t* d_T, uint32_t max_len, uint32_t nb, const uint32_t* lens, const uint32_t* pidx, uint8_t* d_out) {
  std::vector<IbBlock> chain(nb);
  uint64_t M64 = 0;
  for (uint32_t k = 0; k < nb; k++) {
    IbBlock& b = chain[k];
    b.tt = (uint64_t)(uintptr_t)(d_T + M64);
    b.count = lens[k]; b.orig = pidx[k]; b.off = b.woff = (uint32_t)M64; b.out_off = M64; b.out_len = lens[k]; b.crc = 0;
    M64 += lens[k];
  }
  if (M64 >= 0xFFFFF000ull) return CJS_E_UNSUPPORTED;
  const uint32_t M = (uint32_t)M64;
  DevMem<IbBlock> d_blocks;
  DevMem<uint32_t> d_key0, d_key1, d_val0, d_val1, d_snext, d_ssteps, d_srank, d_hist, d_bintot;
  DevMem<int32_t> d_err;
  const uint32_t spl_stride = max_len / SPL + 4;
  const size_t T = ((size_t)M + RS_TILE - 1) / RS_TILE + 1;
  CJS_TRY(d_blocks.alloc(sizeof(IbBlock) * nb));
  CJS_TRY(d_key0.alloc(4 * (size_t)M + 64)); CJS_TRY(d_key1.alloc(4 * (size_t)M + 64));
  CJS_TRY(d_val0.alloc(4 * (size_t)M + 64)); CJS_TRY(d_val1.alloc(4 * (size_t)M + 64));
  CJS_TRY(d_snext.alloc(4 * (size_t)nb * spl_stride)); CJS_TRY(d_ssteps.alloc(4 * (size_t)nb * spl_stride));
  CJS_TRY(d_srank.alloc(4 * (size_t)nb * spl_stride)); CJS_TRY(d_err.alloc(4 * (size_t)nb));
  CJS_TRY(d_hist.alloc(RadixWork::hist_words(T) * 4)); CJS_TRY(d_bintot.alloc(256 * 4));
  RadixWork sw{d_hist, d_bintot, (uint32_t)T, 1u};
  if (hipMemcpyAsync(d_blocks, chain.data(), sizeof(IbBlock) * nb, hipMemcpyHostToDevice, s) != hipSuccess) return CJS_E_HIP;
  hipLaunchKernelGGL(ib_make_keys, dim3(64, nb), dim3(256), 0, s, d_blocks.p, d_key0.p, d_val0.p, 0u);
  int cur = 0;
  CJS_TRY(radix_passes<uint32_t>(s, sw, d_key0, d_val0, d_key1, d_val1, cur, M, 0, 8 + bits_for(nb - 1)));
  uint32_t* sval = cur ? d_val1 : d_val0;
  uint32_t* d_dbuf = cur ? d_key0 : d_key1;
  hipLaunchKernelGGL(ib_pack_sentinel, dim3(64, nb), dim3(256), 0, s, d_blocks.p, sval, d_dbuf);
  const uint32_t cpb = walk_chunks(max_len), wgrid = ((nb * cpb + 7u) >> 3) << 3;
  hipLaunchKernelGGL(ib_walk1, dim3(wgrid), dim3(WALK_T), WALK_LDS, s, d_dbuf, d_blocks.p, nb, cpb, spl_stride, d_snext.p, d_ssteps.p, 1, nullptr, nullptr);
  hipLaunchKernelGGL(ib_rank, dim3(nb), dim3(1024), 0, s, d_blocks.p, nb, spl_stride, d_snext.p, d_ssteps.p, d_srank.p, d_err.p);
  hipLaunchKernelGGL(ib_walk2, dim3(wgrid), dim3(WALK_T), WALK_LDS, s, d_dbuf, d_blocks.p, nb, cpb, spl_stride, d_srank.p, d_ssteps.p, d_out, 1, nullptr, nullptr);
  std::vector<int32_t> errs(nb);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(errs.data(), d_err, 4 * (size_t)nb, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return CJS_E_HIP;
  // The chain visits n distinct rows and then re-enters at row pidx (the step the reference computes last and never
  // uses, BWTC:1163-1165), so the last segment may overshoot; a chain that closes before n rows is corrupt input.
  for (uint32_t k = 0; k < nb; k++) if ((uint32_t)errs[k] < lens[k]) {
    if (env_debug()) fprintf(stderr, "[cjs ibwt] block %u: chain covers %d of %u\n", k, errs[k], lens[k]);
    return CJS_E_DATA_ERROR;
  }
  return 0;
}
int ibwt_sentinel_run(hipStream_t s, const uint8_t* d_T, uint32_t max_len, uint32_t nb, const uint32_t* lens, const uint32_t* pidx, uint8_t* d_out) {
  uint64_t base = 0;
  for (uint32_t k0 = 0; k0 < nb;) {
    uint32_t k1 = k0; uint64_t el = 0;
    while (k1 < nb && k1 - k0 < 65535u && (k1 == k0 || el + lens[k1] <= (1ull << 28))) el += lens[k1++];
    CJS_TRY(ibwt_sentinel_slab(s, d_T + base, max_len, k1 - k0, lens + k0, pidx + k0, d_out + base));
    base += el; k0 = k1;
  }
  return 0;
}
}  // namespace cjs

// ---------------------------------------------------------------- host driver
// mode 0: Bunzip.decode (:1769-1796); mode 1: Bunzip.table (:1823-1863) -> (bit position, size) per block, no bytes;
// mode 2: Bunzip.decodeBlock (:1797-1818) -> the single block whose magic starts at `at_bit`.
//
// The job is cut into per-device shares (SURVEY §8e "Bzip2 decompress"; cjs_opts.n_devices / CJS_DEVICES, one host thread
// per share; several shares may sit on one GPU):
//   A  per share   upload its byte range (+ one worst-case block of overlap), magic scan, speculative decode of every
//                  candidate that STARTS in the share
//   -  host        chain walk 32 -> end(block 0) -> end(block 1) ... over all shares' candidates: stream CRC fold,
//                  multistream restarts (each stream keeps its own level, :1787-1792)
//   B  per share   inverse BWT of the chain blocks it decoded, in batches (bounded scratch), RLE1 length pass
//   -  host        exclusive prefix sum of the decoded lengths -> output offsets
//   C  per share   RLE1 expansion + block CRCs per batch, D2H straight to the final offsets
// No data moves between devices; the exchanged quantities are (end bit, count, crc) per candidate and a length per block.
//
// Five drivers sit on the phases: bunzip_core (single stream, shares over devices), dev_single_* (device-resident single stream),
// dec_batch_group (host batch), dev_group_* (device-resident batch) and dec_step (streaming).  The glue between the phases is
// written once: bz_header_check (_start_bunzip), WalkCands + walk_chain (candidate lookup, bz_walk, chain append),
// chain_out_offsets (the prefix sum), group_layout / group_prepare / group_verdicts (a batch group, both forms), ShareScratch
// (a phase's own scratch).  A driver holds what is particular to it: where the bytes come from and where they go.
namespace {

constexpr uint64_t DEC_BATCH_ELEMS = 1ull << 28;      // BWT bytes per inverse-BWT batch (scratch ~ 21 B each)
constexpr uint32_t DEC_BATCH_BLOCKS = 65535;          // grid.y of the per-block kernels

// Device scratch of one streaming decoder (cjs_bzip2_dec_*): ONE allocation made at the decoder's first step, handed out first fit
// in 256-byte units and taken back piece by piece, so what a decoder holds between its steps never changes.  A request that does
// not fit (the size is an estimate) becomes a hipMalloc of its own, freed when it is given back.
struct DecArena {
  DevMem<uint8_t> base; size_t cap = 0;
  std::vector<std::pair<size_t, size_t>> free_;      // (offset, bytes), ascending, coalesced
  std::vector<std::pair<void*, size_t>> used;        // bytes == 0: a hipMalloc of its own
  uint32_t spills = 0;
  int init(size_t bytes) { CJS_TRY(base.alloc(bytes)); cap = bytes; free_.assign(1, {0, bytes}); return 0; }
  void* take(size_t bytes) {
    bytes = (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
    for (size_t i = 0; i < free_.size(); i++) if (free_[i].second >= bytes) {
      void* p = base.p + free_[i].first;
      if (free_[i].second == bytes) free_.erase(free_.begin() + (long)i); else { free_[i].first += bytes; free_[i].second -= bytes; }
      used.push_back({p, bytes});
      return p;
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    spills++;
    used.push_back({p, 0});
    return p;
  }
  void give(void* p) {
    size_t i = 0;
    while (i < used.size() && used[i].first != p) i++;
    if (i == used.size()) return;
    const size_t bytes = used[i].second, off = bytes ? (size_t)((uint8_t*)p - base.p) : 0;
    used.erase(used.begin() + (long)i);
    if (!bytes) { (void)hipFree(p); return; }
    size_t k = 0;
    while (k < free_.size() && free_[k].first < off) k++;
    free_.insert(free_.begin() + (long)k, {off, bytes});
    if (k + 1 < free_.size() && free_[k].first + free_[k].second == free_[k + 1].first) { free_[k].second += free_[k + 1].second; free_.erase(free_.begin() + (long)k + 1); }
    if (k > 0 && free_[k - 1].first + free_[k - 1].second == free_[k].first) { free_[k - 1].second += free_[k].second; free_.erase(free_.begin() + (long)k); }
  }
  void release() { for (auto& u : used) if (!u.second) (void)hipFree(u.first); used.clear(); free_.clear(); base.reset(); cap = 0; }
  ~DecArena() { release(); }
};

struct DecShare {
  int device = 0, rc = 0;
  Stream s;
  std::vector<DevBuf> bufs;          // device scratch of the share, given back at release() (or early, by drop())
  // a streaming decoder's step: scratch from the decoder's own arena instead of the pool, and rows only for the first row_limit
  // block candidates at or after bit row_from.  Candidates in front of row_from are dropped, as is everything from the first
  // block candidate past the limit on: cut_bit is that candidate's bit (none: ~0).
  DecArena* arena = nullptr; std::vector<void*> abufs;
  uint32_t row_limit = ~0u; uint64_t row_from = 0, cut_bit = ~0ull;
  uint32_t ncand_seen = 0;            // candidates the magic scan found (before the row limit dropped any)
  uint64_t lo = 0, hi = 0;            // candidates starting in bytes [lo, hi) are this share's
  uint64_t up_lo = 0, up_hi = 0;      // uploaded byte range
  const uint8_t* d_in = nullptr;      // addressed by absolute byte: d_in[b] is valid for up_lo <= b < up_hi
  std::vector<Cand> cands;            // sorted by bit
  std::vector<BlockOut> bos;
  uint8_t* d_tt = nullptr;            // decoded BWT bytes of a one-batch share, tt_stride per row (several batches: packed segments)
  std::vector<uint64_t> tt_ptr;       // per candidate: device address of its decoded bytes
  // chain part
  size_t c0 = 0, c1 = 0;              // chain blocks [c0, c1) were decoded here
  uint8_t* d_w = nullptr;             // pre-RLE1 bytes of those blocks, contiguous in chain order
  RleCarry* d_carry = nullptr; uint32_t carry_tiles = 0;      // per chain block and UR_TILE-byte tile: the RLE1 expansion state at the tile start
  std::vector<uint64_t> ebase;        // element offset of block c0+i inside d_w (size c1-c0+1)
  double ms_a = 0, ms_b = 0, ms_c = 0;
  uint64_t h2d = 0, d2h = 0;          // bytes of the share's host <-> device copies
  char detail[96] = {0};            // error detail found by this share's worker thread (the detail text is per calling thread)
  // batch (cjs_bzip2_decompress_batch): input k is bytes [bst[k], ben[k]) of the upload, its blocks at most bdsz[k] bytes
  std::vector<uint32_t> bst, ben, bdsz;
  uint32_t a_batches = 0, b_batches = 0;      // row batches of phase A, inverse-BWT batches of phase B
  int take(void** p, size_t bytes) {
    if (arena) { if (!(*p = arena->take(bytes))) return (int)CJS_E_OUT_OF_MEMORY; abufs.push_back(*p); return 0; }
    DevBuf b(bytes); if (!(*p = b.p)) return (int)CJS_E_OUT_OF_MEMORY; bufs.push_back(std::move(b)); return 0;
  }
  void drop(void* p) {
    if (arena) { for (size_t i = 0; i < abufs.size(); i++) if (abufs[i] == p) { abufs.erase(abufs.begin() + (long)i); arena->give(p); return; } return; }
    for (size_t i = 0; i < bufs.size(); i++) if (bufs[i].p == p) { bufs.erase(bufs.begin() + (long)i); return; }
  }
  void release() {                    // on the share's device, once its stream has drained; again: nothing
    if (hipSetDevice(device) != hipSuccess) return;
    if (s) (void)hipStreamSynchronize(s);
    if (arena) for (void* p : abufs) arena->give(p);
    abufs.clear();
    bufs.clear();
    s.reset();
  }
  void release_keep_stream(Stream& to) { Stream keep = std::move(s); if (keep && hipSetDevice(device) == hipSuccess) (void)hipStreamSynchronize(keep); release(); to = std::move(keep); }
  uint32_t nrows_given() const { uint32_t r = 0; for (auto& c : cands) r += c.kind == 0; return r; }
  ~DecShare() { release(); }
};

// Scratch a phase takes from its share for its own duration.  done() gives all of it back, and is called only where the share's
// stream has been synchronised behind the last kernel that used it (another thread may get the memory at once).  On an error exit
// nothing goes back: the buffers stay with the share until DecShare::release(), which synchronises first.  So no destructor.
struct ShareScratch {
  DecShare* S; std::vector<void*> got;
  explicit ShareScratch(DecShare* s) : S(s) {}
  int take(void** p, size_t bytes) { const int rc = S->take(p, bytes); if (!rc) got.push_back(*p); return rc; }
  void drop(void* p) { got.erase(std::find(got.begin(), got.end(), p)); S->drop(p); }      // one buffer, early
  void done() { for (void* p : got) S->drop(p); got.clear(); }
};

struct DecJob {
  const uint8_t* in = nullptr; size_t n = 0;
  uint32_t tt_stride = 0;             // = dbuf size of the largest level in the input
  int mode = 0;
  std::vector<IbBlock> chain;         // all valid blocks in stream order (cand = index local to the decoding share)
  std::vector<uint64_t> chain_bits;
  std::vector<uint64_t> out_off;      // size chain.size()+1
  uint8_t* host = nullptr;            // final output (mode 0 / 2)
  bool timing = false;
  bool batch = false;                 // phase C: a CRC verdict for every block (crc_got) instead of stopping at the first bad one
  std::vector<uint32_t> crc_got;
  // device-resident source and sink (cjs_bzip2_decompress_device[_batch]).  upload: fills the share's scratch [0, up_hi - up_lo)
  // on its stream in place of phase A's H2D of `in`; eos: called once phase A's candidates are sorted (a batch candidate's pad
  // still names its input); dev_out: phase C expands straight into dev_out at the final offsets instead of scratch + D2H
  std::function<int(DecShare* S, uint8_t* dst)> upload;
  std::function<int(DecShare* S)> eos;
  uint8_t* dev_out = nullptr;
  // range reads: the share comes with its candidates (S->cands, sorted, kind 0) and phase A launches no magic scan.  vet, if
  // set, is called once the upload is enqueued and may erase candidates (those whose magic is not there)
  bool given = false;
  std::function<int(DecShare* S)> vet;
};

double ms_since(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); }

// ---- phase A
void dec_phase_a(DecJob* J, DecShare* S) {
  const auto T0 = std::chrono::steady_clock::now();
  if (hipSetDevice(S->device) != hipSuccess || (!S->s && hipStreamCreate(S->s.put()) != hipSuccess)) { S->rc = CJS_E_HIP; return; }      // (a device source made it for the header pass)
  hipStream_t s = S->s;
  const size_t up_n = (size_t)(S->up_hi - S->up_lo);
  uint8_t* d_raw = nullptr; Cand* d_cand = nullptr; uint32_t* d_count = nullptr;
  uint32_t cand_cap = J->given ? (uint32_t)S->cands.size() + 1u : (uint32_t)((S->hi - S->lo) / 64 + 1024);      // grown to the exact count if a file of tiny streams has more
  ShareScratch q(S);                                                    // (the upload stays with the share)
  int rc = S->take((void**)&d_raw, up_n + 256 + 16);
  if (!rc) rc = q.take((void**)&d_cand, sizeof(Cand) * cand_cap);
  if (!rc) rc = q.take((void**)&d_count, 64);
  if (rc) { S->rc = rc; return; }
  // keep the dword phase of the stream: the decoders fetch aligned big-endian words by absolute word index
  uint8_t* d_al = d_raw + (S->up_lo & 3u);
  S->d_in = d_al - S->up_lo;
  if (J->upload) rc = J->upload(S, d_al);                               // (a device source: its own copy or gather)
  else if (hipMemcpyAsync(d_al, J->in + S->up_lo, up_n, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
  else S->h2d += up_n;
  if (rc || hipMemsetAsync(d_count, 0, 64, s) != hipSuccess) { S->rc = rc ? rc : CJS_E_HIP; return; }
  uint32_t *d_bst = nullptr, *d_ben = nullptr;
  const uint32_t nin = (uint32_t)S->bst.size();
  if (nin) {
    if ((rc = q.take((void**)&d_bst, 4 * (size_t)nin)) != 0 || (rc = q.take((void**)&d_ben, 4 * (size_t)nin)) != 0) { S->rc = rc; return; }
    if (hipMemcpyAsync(d_bst, S->bst.data(), 4 * (size_t)nin, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_ben, S->ben.data(), 4 * (size_t)nin, hipMemcpyHostToDevice, s) != hipSuccess) { S->rc = CJS_E_HIP; return; }
    S->h2d += 8 * (size_t)nin;
  }
  auto launch_scan = [&]() {                                            // (slabs: a grid may not exceed 2^32 threads)
    if (nin) { launch_magic_scan_batch(s, S->d_in, d_bst, d_ben, nin, S->hi, d_cand, cand_cap, d_count); return; }
    for (uint64_t b0 = S->lo; b0 < S->hi; b0 += 1ull << 31) {
      const uint64_t b1 = std::min<uint64_t>(S->hi, b0 + (1ull << 31));
      hipLaunchKernelGGL(bz_magic_scan, dim3((unsigned)((b1 - b0 + 255) / 256)), dim3(256), 0, s, S->d_in, b0, b1, S->up_hi, d_cand, cand_cap, d_count);
    }
  };
  uint32_t ncand = (uint32_t)S->cands.size();
  if (!J->given) {
    launch_scan();
    ncand = 0;
    if (hipMemcpyAsync(&ncand, d_count, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { S->rc = CJS_E_HIP; return; }
    S->d2h += 4;
    if (ncand > cand_cap) {                                             // more magics than planned for (many tiny member streams): scan again with room for all
      q.drop(d_cand);
      cand_cap = ncand;
      if ((rc = q.take((void**)&d_cand, sizeof(Cand) * cand_cap)) != 0) { S->rc = rc; return; }
      if (hipMemsetAsync(d_count, 0, 64, s) != hipSuccess) { S->rc = CJS_E_HIP; return; }
      launch_scan();
      if (hipMemcpyAsync(&ncand, d_count, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { S->rc = CJS_E_HIP; return; }
      S->d2h += 4;
      if (ncand > cand_cap) { S->rc = CJS_E_HIP; return; }
    }
    S->cands.resize(ncand);
    if (ncand && hipMemcpy(S->cands.data(), d_cand, sizeof(Cand) * ncand, hipMemcpyDeviceToHost) != hipSuccess) { S->rc = CJS_E_HIP; return; }
    S->d2h += sizeof(Cand) * (size_t)ncand;
    std::sort(S->cands.begin(), S->cands.end(), [](const Cand& a, const Cand& b) { return a.bit < b.bit; });
    S->ncand_seen = ncand;
  } else if (J->vet) {
    if ((rc = J->vet(S)) != 0) { S->rc = rc; return; }
    ncand = (uint32_t)S->cands.size();
  }
  if (S->row_limit != ~0u) {                                          // (a streaming step: see DecShare)
    size_t a = 0, b;
    while (a < S->cands.size() && S->cands[a].bit < S->row_from) a++;
    uint32_t blocks = 0;
    for (b = a; b < S->cands.size(); b++) if (S->cands[b].kind == 0 && ++blocks > S->row_limit) { S->cut_bit = S->cands[b].bit; break; }
    S->cands.erase(S->cands.begin() + (long)b, S->cands.end());
    S->cands.erase(S->cands.begin(), S->cands.begin() + (long)a);
    ncand = (uint32_t)S->cands.size();
  }
  if (J->eos && ncand && (rc = J->eos(S)) != 0) { S->rc = rc; return; }
  uint32_t* d_cend = nullptr;                                      // batch: per candidate, its input's end and block size (cend, then cdsz)
  if (nin && ncand) {                                              // the batch scan left each candidate's input in pad
    std::vector<uint32_t> cend(2 * (size_t)ncand);
    for (uint32_t c = 0; c < ncand; c++) { cend[c] = S->ben[S->cands[c].pad]; cend[ncand + c] = S->bdsz[S->cands[c].pad]; }
    if ((rc = q.take((void**)&d_cend, 8 * (size_t)ncand)) != 0) { S->rc = rc; return; }
    if (hipMemcpy(d_cend, cend.data(), 8 * (size_t)ncand, hipMemcpyHostToDevice) != hipSuccess) { S->rc = CJS_E_HIP; return; }
    S->h2d += 8 * (size_t)ncand;
  }
  uint32_t nrows = 0;                                              // only block candidates get a row of the decode buffer
  for (auto& c : S->cands) c.pad = c.kind == 0 ? nrows++ : 0u;
  if (ncand && hipMemcpy(d_cand, S->cands.data(), sizeof(Cand) * ncand, hipMemcpyHostToDevice) != hipSuccess) { S->rc = CJS_E_HIP; return; }
  S->h2d += sizeof(Cand) * (size_t)ncand;
  S->bos.resize(ncand);
  S->tt_ptr.assign(ncand, 0ull);
  if (!ncand) { S->ms_a = ms_since(T0); return; }
  // Block decode in three stages (Huffman chain per block -> (rank, offset) ops; move-to-front of all 256-op tiles in parallel;
  // emit), over BATCHES of rows: a row of scratch is sized for a whole block of the file's largest level (~7 x tt_stride bytes),
  // whatever the candidate turns out to hold, so a file of very many tiny member streams (or one stuffed with block magics)
  // must not get a row per candidate at once.  One batch (the usual case: <= ~2000 level-9 rows in 16 GiB: a 2^30-byte stream has 1,194) keeps its decoded
  // rows where they are; with several batches each batch's decoded bytes are packed into a buffer of their exact size and
  // the scratch rows are used again.
  BlockOut* d_bo = nullptr;
  const uint32_t dsz = J->tt_stride;
  const uint32_t ops_stride = (dsz + 256u + 255u) & ~255u, tiles_per_row = ops_stride / MT_TILE;
  static const uint64_t budget = getenv("CJS_DEC_ROW_BYTES") ? strtoull(getenv("CJS_DEC_ROW_BYTES"), nullptr, 10) : (16ull << 30);      // (tests shrink it)
  const uint32_t sym_stride = dsz + 4096u;                              // symbols in front of the end of block: each emits a byte (but for forgotten runs), so <= dsz
  const uint32_t group_tiles = (std::min<uint32_t>(MAX_SELECTORS, sym_stride / GROUP_SYMS + 1u) + 255u) / 256u;
  const uint32_t sym_groups = (sym_stride + GROUP_SYMS - 1) / GROUP_SYMS;
  const uint64_t per_row = (uint64_t)dsz + 6ull * ops_stride + 256 + 4 + sizeof(RowTab) + MAX_SELECTORS + 4ull * (MAX_SELECTORS + 1) + 2ull * sym_groups * GROUP_SYMS;
  const uint32_t nr = std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>(std::min<uint64_t>(nrows ? nrows : 1u, 65535u), std::max<uint64_t>(1ull, budget / per_row)));      // (<= grid.y)
  const bool single = nrows <= nr;
  uint8_t *d_ttb = nullptr, *d_ops = nullptr, *d_l0 = nullptr, *d_pl = nullptr, *d_sel = nullptr; uint32_t *d_opoff = nullptr, *d_nops = nullptr, *d_gstart = nullptr;
  RowDst* d_gdst = nullptr; RowTab* d_tabs = nullptr; uint16_t* d_syms = nullptr;
  rc = single ? S->take((void**)&d_ttb, (size_t)nr * dsz) : q.take((void**)&d_ttb, (size_t)nr * dsz);      // (one batch: the rows are phase B's input)
  if (!rc) rc = q.take((void**)&d_bo, sizeof(BlockOut) * ncand);
  if (!rc) rc = q.take((void**)&d_ops, (size_t)nr * ops_stride);
  if (!rc) rc = q.take((void**)&d_opoff, 4 * (size_t)nr * ops_stride);
  if (!rc) rc = q.take((void**)&d_l0, (size_t)nr * 256);
  if (!rc) rc = q.take((void**)&d_pl, (size_t)nr * ops_stride);
  if (!rc) rc = q.take((void**)&d_nops, 4 * (size_t)nr);
  if (!rc) rc = q.take((void**)&d_tabs, sizeof(RowTab) * (size_t)nr);
  if (!rc) rc = q.take((void**)&d_sel, (size_t)MAX_SELECTORS * nr);
  if (!rc) rc = q.take((void**)&d_gstart, 4 * (size_t)(MAX_SELECTORS + 1) * nr);
  if (!rc) rc = q.take((void**)&d_syms, 2 * (size_t)sym_groups * GROUP_SYMS * nr);
  if (!rc && !single) rc = q.take((void**)&d_gdst, sizeof(RowDst) * (size_t)nr);
  uint32_t* d_rlim = nullptr;
  if (!rc && nin) rc = q.take((void**)&d_rlim, 4 * (size_t)nr);
  if (rc) { S->rc = rc; return; }
  if (single) S->d_tt = d_ttb;
  std::vector<RowDst> gdst(single ? 0 : nr);
  for (uint32_t c0 = 0; c0 < ncand;) {
    // candidates [c0, c1): at most nr block candidates (rows r0 .. r0 + rows)
    uint32_t c1 = c0, rows = 0, r0 = 0;
    while (c1 < ncand && (S->cands[c1].kind != 0 || rows < nr)) { if (S->cands[c1].kind == 0) { if (!rows) r0 = S->cands[c1].pad; rows++; } c1++; }
    const uint32_t nc = c1 - c0;
    S->a_batches++;
    if (nin) launch_block_decode_batch(s, S->d_in, d_cend + c0, d_cend + ncand + c0, d_rlim, d_cand + c0, nc, rows, dsz, d_tabs, d_sel, d_gstart, d_l0, d_bo + c0, r0, group_tiles, d_syms, sym_stride,
                                       sym_groups, d_ops, d_opoff, ops_stride, d_nops);
    else {
      hipLaunchKernelGGL(bz_chain, dim3(nc), dim3(CH_T), 0, s, S->d_in, S->up_hi, d_cand + c0, nc, dsz, d_tabs, d_sel, d_gstart, d_l0, d_bo + c0, r0);
      if (rows) hipLaunchKernelGGL(bz_group_syms, dim3(group_tiles, rows), dim3(256), 0, s, S->d_in, S->up_hi, d_tabs, d_sel, d_gstart, d_syms, sym_stride, sym_groups, 0u);
      hipLaunchKernelGGL(bz_sym_ops, dim3(nc), dim3(1024), 0, s, d_tabs, d_cand + c0, nc, d_syms, sym_groups, dsz, d_ops, d_opoff, ops_stride, d_nops, d_bo + c0, r0, S->up_hi * 8);
    }
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(S->bos.data() + c0, d_bo + c0, sizeof(BlockOut) * nc, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) { S->rc = CJS_E_HIP; return; }
    S->d2h += sizeof(BlockOut) * (size_t)nc;
    uint32_t maxc = 0; uint64_t packed = 0;
    for (uint32_t c = c0; c < c1; c++) if (S->cands[c].kind == 0 && !S->bos[c].err) { maxc = std::max(maxc, S->bos[c].count); packed += ((uint64_t)S->bos[c].count + 15u) & ~15ull; }
    if (rows) {
      const uint32_t tiles_used = std::min<uint32_t>(maxc / MT_TILE + 1u, tiles_per_row);
      // slabs of rows: grid.y <= 65535 and grid.x * grid.y * 256 threads < 2^32 (a larger launch is cut short without an error)
      const uint32_t slab = std::min<uint32_t>(65535u, std::max<uint32_t>(1u, (1u << 23) / tiles_used));
      for (uint32_t q0 = 0; q0 < rows; q0 += slab)
        hipLaunchKernelGGL(bz_mtf_tiles, dim3((tiles_used + 3u) / 4u, std::min(slab, rows - q0)), dim3(256), 0, s, d_ops, ops_stride, d_nops, d_pl, tiles_per_row, q0);
      {                                                                // (the symbols are spent: their rows hold the chunks' products)
        const uint32_t chunks = (tiles_used + MC_TILES - 1) / MC_TILES;
        const size_t cstride = 2 * (size_t)sym_groups * GROUP_SYMS;
        hipLaunchKernelGGL(bz_mtf_chunk_perm, dim3(chunks, rows), dim3(256), 0, s, d_nops, d_pl, tiles_per_row, reinterpret_cast<uint8_t*>(d_syms), cstride);
        hipLaunchKernelGGL(bz_mtf_compose, dim3(chunks, rows), dim3(256), 0, s, d_nops, d_l0, d_pl, tiles_per_row, reinterpret_cast<const uint8_t*>(d_syms), cstride);
      }
      for (uint32_t q0 = 0; q0 < rows; q0 += slab)
        hipLaunchKernelGGL(bz_mtf_emit, dim3(tiles_used, std::min(slab, rows - q0)), dim3(256), 0, s, d_ops, d_opoff, ops_stride, d_nops, d_l0, d_pl, tiles_per_row, q0, d_ttb, dsz);
      if (hipGetLastError() != hipSuccess) { S->rc = CJS_E_HIP; return; }
      if (single) {
        for (uint32_t c = c0; c < c1; c++) if (S->cands[c].kind == 0) S->tt_ptr[c] = (uint64_t)(uintptr_t)(d_ttb + (size_t)(S->cands[c].pad - r0) * dsz);
      } else {
        uint8_t* seg = nullptr;                                        // (kept until the share is released)
        if ((rc = S->take((void**)&seg, (size_t)packed + 16)) != 0) { S->rc = rc; return; }
        uint64_t at = 0;
        for (uint32_t c = c0; c < c1; c++) if (S->cands[c].kind == 0) {
          const uint32_t row = S->cands[c].pad - r0, cnt = S->bos[c].err ? 0u : S->bos[c].count;
          gdst[row] = RowDst{(uint64_t)(uintptr_t)(seg + at), cnt};
          S->tt_ptr[c] = (uint64_t)(uintptr_t)(seg + at);
          at += ((uint64_t)cnt + 15u) & ~15ull;
        }
        if (hipMemcpyAsync(d_gdst, gdst.data(), sizeof(RowDst) * (size_t)rows, hipMemcpyHostToDevice, s) != hipSuccess) { S->rc = CJS_E_HIP; return; }
        S->h2d += sizeof(RowDst) * (size_t)rows;
        hipLaunchKernelGGL(bz_rows_pack, dim3(16, rows), dim3(256), 0, s, d_ttb, dsz, d_gdst);
        if (hipGetLastError() != hipSuccess) { S->rc = CJS_E_HIP; return; }
      }
      if (hipStreamSynchronize(s) != hipSuccess) { S->rc = CJS_E_HIP; return; }
    }
    c0 = c1;
  }
  if (env_debug()) {
    uint64_t clk[8];
    if (!nin && hipMemcpyFromSymbol(clk, HIP_SYMBOL(g_dec_clk), sizeof clk) == hipSuccess) {
      S->d2h += sizeof clk;
      fprintf(stderr, "[cjs dec] candidate 0: header + tables %.1f us, group chain %.1f us for %llu groups\n", clk[5] / 100.0, clk[6] / 100.0, (unsigned long long)clk[7]);
    }
    fprintf(stderr, "[cjs dec] share on device %d: bytes [%llu, %llu) uploaded [%llu, %llu) = %zu B, %u candidates\n", S->device, (unsigned long long)S->lo,
            (unsigned long long)S->hi, (unsigned long long)S->up_lo, (unsigned long long)S->up_hi, up_n, ncand);
  }
  q.done();                                                             // (every batch ended with the stream drained)
  S->ms_a = ms_since(T0);
}

// scratch of one inverse-BWT batch
struct IbScratch {
  IbBlock* d_blocks = nullptr; uint32_t *key0 = nullptr, *key1 = nullptr, *val0 = nullptr, *val1 = nullptr;
  uint32_t *snext = nullptr, *ssteps = nullptr, *srank = nullptr, *resume = nullptr; int32_t* d_err = nullptr;
  uint8_t* seg = nullptr;      // ib_walk1's kept bytes: SEG_CAP per splitter
  RadixWork sw;
};

// batches of the share's chain blocks: [b0, b1) with <= DEC_BATCH_ELEMS elements and <= DEC_BATCH_BLOCKS blocks
size_t dec_next_batch(const DecJob* J, size_t b0, size_t c1) {
  static const uint64_t max_el = getenv("CJS_DEC_BATCH_ELEMS") ? strtoull(getenv("CJS_DEC_BATCH_ELEMS"), nullptr, 10) : DEC_BATCH_ELEMS;   // (tests shrink it)
  uint64_t el = 0; size_t b = b0;
  while (b < c1 && b - b0 < DEC_BATCH_BLOCKS && (b == b0 || el + J->chain[b].count <= max_el)) { el += J->chain[b].count; b++; }
  return b;
}

// ---- phase B: inverse BWT (T vector by a stable radix pass, splitter list ranking, second walk) + RLE1 length pass
void dec_phase_b(DecJob* J, DecShare* S) {
  if (S->c1 <= S->c0) return;
  const auto T0 = std::chrono::steady_clock::now();
  if (hipSetDevice(S->device) != hipSuccess) { S->rc = CJS_E_HIP; return; }
  hipStream_t s = S->s;
  const size_t nbk = S->c1 - S->c0;
  S->ebase.assign(nbk + 1, 0);
  for (size_t i = 0; i < nbk; i++) S->ebase[i + 1] = S->ebase[i] + J->chain[S->c0 + i].count;
  int rc = S->take((void**)&S->d_w, (size_t)S->ebase[nbk] + 64);
  S->carry_tiles = (J->tt_stride + UR_TILE - 1) / UR_TILE;              // RLE1 state carried into every tile: written by phase B, read by phase C
  if (!rc) rc = S->take((void**)&S->d_carry, sizeof(RleCarry) * (size_t)nbk * S->carry_tiles);
  if (rc) { S->rc = rc; return; }
  for (size_t b0 = S->c0; b0 < S->c1 && !rc;) {
    const size_t b1 = dec_next_batch(J, b0, S->c1);
    const uint32_t nb = (uint32_t)(b1 - b0);
    S->b_batches++;
    const uint64_t e0 = S->ebase[b0 - S->c0], M64 = S->ebase[b1 - S->c0] - e0;
    if (M64 >= 0xFFFFF000ull) { rc = CJS_E_UNSUPPORTED; break; }     // a single block list beyond the batch limit cannot happen (count <= 900000)
    // Blocks of (nearly) one size -- a stream's are, but for its last -- get a slot range of that size each and ONE pass of the sort,
    // segment by segment; otherwise the block number is sorted on too (one or two more passes over everything).
    uint32_t maxc = 0;
    for (size_t k = b0; k < b1; k++) maxc = std::max(maxc, J->chain[k].count);
    const uint32_t seg_stride = (maxc + 3u) & ~3u;
    const uint32_t spl_stride = maxc / SPL + 4;                      // (of this batch: a file of very many small blocks must not pay for the largest level's)
    const bool strided = (uint64_t)nb * seg_stride <= M64 + M64 / 4 && (uint64_t)nb * seg_stride < 0xFFFFF000ull;
    const uint32_t M = strided ? nb * seg_stride : (uint32_t)M64;
    for (size_t k = b0; k < b1; k++) {
      J->chain[k].woff = (uint32_t)(S->ebase[k - S->c0] - e0);
      J->chain[k].off = strided ? (uint32_t)(k - b0) * seg_stride : J->chain[k].woff;
    }
    IbScratch q; ShareScratch g(S);
    rc = g.take((void**)&q.d_blocks, sizeof(IbBlock) * nb);
    if (!rc) rc = g.take((void**)&q.key0, 4 * (size_t)M + 64); if (!rc) rc = g.take((void**)&q.key1, 4 * (size_t)M + 64);
    if (!strided) { if (!rc) rc = g.take((void**)&q.val0, 4 * (size_t)M + 64); if (!rc) rc = g.take((void**)&q.val1, 4 * (size_t)M + 64); }
    if (!rc) rc = g.take((void**)&q.snext, 4 * (size_t)nb * spl_stride); if (!rc) rc = g.take((void**)&q.ssteps, 4 * (size_t)nb * spl_stride);
    if (!rc) rc = g.take((void**)&q.srank, 4 * (size_t)nb * spl_stride); if (!rc) rc = g.take((void**)&q.d_err, 4 * (size_t)nb);
    if (!rc) rc = g.take((void**)&q.resume, 4 * (size_t)nb * spl_stride);
    // (the first walk's kept bytes: without them -- one large block among very many tiny ones would ask for SEG_CAP x 14,066 bytes for
    // each -- the second walk does all the work, as it does for the sentinel form)
    const uint64_t seg_bytes = (uint64_t)nb * spl_stride * SEG_CAP;
    if (!rc && seg_bytes <= (8ull << 30) && g.take((void**)&q.seg, (size_t)seg_bytes) != 0) q.seg = nullptr;
    const uint32_t tps = (seg_stride + RS_TILE - 1) / RS_TILE;
    const size_t T = strided ? (size_t)nb * tps + 1 : ((size_t)M + RS_TILE - 1) / RS_TILE + 1;
    if (!rc) rc = g.take((void**)&q.sw.hist, RadixWork::hist_words(T) * 4); if (!rc) rc = g.take((void**)&q.sw.bintot, 256 * 4 * (size_t)(strided ? nb : 1u));
    q.sw.hist_tiles = (uint32_t)T; q.sw.bintot_segs = strided ? nb : 1u;
    if (!rc && hipMemcpyAsync(q.d_blocks, J->chain.data() + b0, sizeof(IbBlock) * nb, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
    if (!rc && hipMemsetAsync(q.d_err, 0, 4 * (size_t)nb, s) != hipSuccess) rc = CJS_E_HIP;
    if (rc) break;
    uint8_t* d_wb = S->d_w + e0;
    if (strided) hipLaunchKernelGGL(ib_make_keys_hist, dim3(tps, nb), dim3(256), 0, s, q.d_blocks, q.key0, seg_stride, tps, q.sw.hist);
    else hipLaunchKernelGGL(ib_make_keys, dim3(64, nb), dim3(256), 0, s, q.d_blocks, q.key0, q.val0, 0u);
    int cur = 0;
    if (strided) rc = radix_pass_segments(s, q.sw, q.key0, q.val0, q.key1, q.val1, cur, nb, seg_stride, 0, 8, true, true);
    else rc = radix_passes<uint32_t>(s, q.sw, q.key0, q.val0, q.key1, q.val1, cur, M, 0, 8 + bits_for(nb - 1));
    if (rc) break;
    const uint32_t* sval = strided ? (cur ? q.key1 : q.key0) : (cur ? q.val1 : q.val0);      // (strided: the sorted keys carry the indices)
    uint32_t* d_dbuf = cur ? q.key0 : q.key1;                      // the buffer the sort is not sitting in
    hipLaunchKernelGGL(ib_pack, dim3(64, nb), dim3(256), 0, s, q.d_blocks, sval, d_dbuf, strided ? 1 : 0);
    const uint32_t cpb = walk_chunks(maxc), wgrid = ((nb * cpb + 7u) >> 3) << 3;
    hipLaunchKernelGGL(ib_walk1, dim3(wgrid), dim3(WALK_T), WALK_LDS, s, d_dbuf, q.d_blocks, nb, cpb, spl_stride, q.snext, q.ssteps, 0, q.seg, q.resume);
    hipLaunchKernelGGL(ib_rank, dim3(nb), dim3(1024), 0, s, q.d_blocks, nb, spl_stride, q.snext, q.ssteps, q.srank, q.d_err);
    // (placing inside the second walk, whose workgroups are few per CU, was no faster than the two launches: 0.49 vs 0.21 + 0.26 ms)
    if (q.seg) hipLaunchKernelGGL(ib_place, dim3((spl_stride + 255) / 256, nb), dim3(256), 0, s, q.d_blocks, spl_stride, q.srank, q.ssteps, q.seg, d_wb);
    hipLaunchKernelGGL(ib_walk2, dim3(wgrid), dim3(WALK_T), WALK_LDS, s, d_dbuf, q.d_blocks, nb, cpb, spl_stride, q.srank, q.ssteps, d_wb, 0, q.resume, q.seg);
    hipLaunchKernelGGL(ib_periodic_fill, dim3(32, nb), dim3(256), 0, s, q.d_blocks, q.d_err, d_wb);
    {
      RleCarry* cr = S->d_carry + (size_t)(b0 - S->c0) * S->carry_tiles;
      hipLaunchKernelGGL(unrle1_bounds, dim3(S->carry_tiles, nb), dim3(1024), 0, s, d_wb, q.d_blocks, cr, S->carry_tiles);
      hipLaunchKernelGGL(unrle1_sums, dim3(S->carry_tiles, nb), dim3(1024), 0, s, d_wb, q.d_blocks, cr, S->carry_tiles);
      hipLaunchKernelGGL(unrle1_carries, dim3(nb), dim3(64), 0, s, q.d_blocks, cr, S->carry_tiles);
    }
    std::vector<int32_t> errs(nb);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(J->chain.data() + b0, q.d_blocks, sizeof(IbBlock) * nb, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(errs.data(), q.d_err, 4 * (size_t)nb, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { rc = CJS_E_HIP; break; }
    S->h2d += sizeof(IbBlock) * (size_t)nb; S->d2h += (sizeof(IbBlock) + 4) * (size_t)nb;
    for (uint32_t k = 0; k < nb; k++) if (errs[k] <= 0) rc = CJS_E_DATA_ERROR;      // cannot happen: the walk makes >= 1 step
    g.done();
    b0 = b1;
  }
  if (S->d_tt) { S->drop(S->d_tt); S->d_tt = nullptr; }
  S->rc = rc;
  S->ms_b = ms_since(T0);
}

// Bad block CRC (:1756-1761): the detail text
void bad_crc_detail(char* d, size_t cap, uint32_t got, uint32_t expected) { snprintf(d, cap, "Bad block CRC (got %x expected %x)", got, expected); }

// ---- phase C: RLE1 expansion to the final byte offsets, block CRC check, D2H
void dec_phase_c(DecJob* J, DecShare* S) {
  if (S->c1 <= S->c0) return;
  const auto T0 = std::chrono::steady_clock::now();
  if (hipSetDevice(S->device) != hipSuccess) { S->rc = CJS_E_HIP; return; }
  hipStream_t s = S->s;
  int rc = 0;
  for (size_t b0 = S->c0; b0 < S->c1 && !rc;) {
    const size_t b1 = dec_next_batch(J, b0, S->c1);
    const uint32_t nb = (uint32_t)(b1 - b0);
    const uint64_t e0 = S->ebase[b0 - S->c0], o0 = J->out_off[b0], obytes = J->out_off[b1] - o0;
    std::vector<IbBlock> blk(J->chain.begin() + (long)b0, J->chain.begin() + (long)b1);
    uint32_t need_segs = 1;
    for (uint32_t k = 0; k < nb; k++) {
      blk[k].off = blk[k].woff = (uint32_t)(S->ebase[b0 + k - S->c0] - e0);
      blk[k].out_off = J->out_off[b0 + k] - o0;                   // inside the batch's output buffer
      const uint32_t sg = (uint32_t)((blk[k].out_len + 16383) / 16384 + 1);
      if (sg > need_segs) need_segs = sg;
    }
    // (a device sink: unrle1_write stores only inside [out_off, out_off + out_len) of each block, crc_ranges reads aligned 16-byte
    // pieces that hold a byte of the range: the caller's buffer takes the bytes at their final offsets)
    IbBlock* d_blocks = nullptr; uint8_t* d_out = J->dev_out ? J->dev_out + o0 : nullptr; RleBlock* d_ranges = nullptr; uint32_t *d_nb = nullptr, *d_seg = nullptr, *d_crc = nullptr;
    ShareScratch g(S);
    rc = g.take((void**)&d_blocks, sizeof(IbBlock) * nb);
    if (!rc && !J->dev_out) rc = g.take((void**)&d_out, (size_t)obytes + 64);
    if (!rc) rc = g.take((void**)&d_ranges, sizeof(RleBlock) * nb);
    if (!rc) rc = g.take((void**)&d_nb, 64);
    if (!rc) rc = g.take((void**)&d_seg, 4 * (size_t)nb * need_segs);
    if (!rc) rc = g.take((void**)&d_crc, 4 * (size_t)nb);
    if (!rc && hipMemcpyAsync(d_blocks, blk.data(), sizeof(IbBlock) * nb, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
    if (rc) break;
    hipLaunchKernelGGL(unrle1_write, dim3(S->carry_tiles, nb), dim3(1024), 0, s, S->d_w + e0, d_blocks, S->d_carry + (size_t)(b0 - S->c0) * S->carry_tiles, S->carry_tiles, d_out);
    hipLaunchKernelGGL(ib_make_crc_ranges, dim3((nb + 63) / 64), dim3(64), 0, s, d_blocks, nb, d_ranges, d_nb);
    rc = crc_ranges(s, d_out, d_ranges, d_nb, nb, need_segs, d_seg, d_crc);
    std::vector<uint32_t> crcs(nb);
    if (!rc && hipMemcpyAsync(crcs.data(), d_crc, 4 * (size_t)nb, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
    if (!rc && J->host && obytes && hipMemcpyAsync(J->host + o0, d_out, (size_t)obytes, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = CJS_E_HIP;
    if (!rc) { S->h2d += sizeof(IbBlock) * (size_t)nb; S->d2h += 4 * (size_t)nb + (J->host ? (size_t)obytes : 0); }
    if (!rc && J->batch) for (uint32_t k = 0; k < nb; k++) J->crc_got[b0 + k] = crcs[k];      // (each input's verdict: the batch's host side)
    else if (!rc) for (uint32_t k = 0; k < nb; k++) if (crcs[k] != blk[k].crc) {                    // Bad block CRC (:1756-1761)
      bad_crc_detail(S->detail, sizeof S->detail, crcs[k], blk[k].crc);
      if (env_debug()) fprintf(stderr, "[cjs dec] block %zu: Bad block CRC (got %08x expected %08x) out_len %u\n", b0 + k, crcs[k], blk[k].crc, blk[k].out_len);
      rc = CJS_E_DATA_ERROR; break;
    }
    g.done();
    b0 = b1;
  }
  S->rc = rc;
  S->ms_c = ms_since(T0);
}

template <typename F>
int for_each_share(std::vector<DecShare>& sh, DecJob* J, F fn) {
  // an exception of a phase becomes the share's return code
  if (sh.size() == 1) guarded(sh[0].rc, [&] { fn(J, &sh[0]); });
  else { Workers workers; for (auto& x : sh) workers.run(x.rc, [fn, J, &x] { fn(J, &x); }); }      // (joined here)
  for (auto& x : sh) if (x.rc) { if (x.detail[0]) set_detail("%s", x.detail); return x.rc; }
  return 0;
}

// _start_bunzip (:1408-1427) on the first four bytes h of an input (or of a member stream) of n bytes: 0 and the level, or
// CJS_E_NOT_BZIP_DATA and the detail text in *why (the caller sets it, or stores it with its input)
int bz_header_check(const uint8_t* h, size_t n, int* level, const char** why) {
  if (n < 4 || h[0] != 'B' || h[1] != 'Z' || h[2] != 'h') { *why = "bad magic"; return CJS_E_NOT_BZIP_DATA; }
  *level = h[3] - '0';
  if (*level < 1 || *level > 9) { *why = "level out of range"; return CJS_E_NOT_BZIP_DATA; }
  return 0;
}

// bytes a block can span: 20 bits per symbol + tables (the overlap of two shares; a streaming decoder's window behind a chunk)
constexpr uint64_t dec_extent(uint32_t tt_stride) { return (uint64_t)tt_stride * 5 / 2 + 65536; }

// The scratch rows are sized for the largest level any member stream can have: a multistream file may change level
// between members (:1787-1792), so every byte-aligned "BZh<d>" followed by a block or end-of-stream magic counts.
int bz_max_level(const uint8_t* in, size_t n, int level, bool multistream) {
  int max_level = level;
  if (multistream) {
    for (const uint8_t* p = in + 4; p + 10 <= in + n && (p = (const uint8_t*)memchr(p, 'B', (size_t)(in + n - 9 - p))) != nullptr; p++) {
      if (p[1] != 'Z' || p[2] != 'h' || p[3] < '1' || p[3] > '9') continue;
      uint64_t m = 0; for (int i = 0; i < 6; i++) m = (m << 8) | p[4 + i];
      if ((m == MAGIC_BLOCK || m == MAGIC_END) && p[3] - '0' > max_level) max_level = p[3] - '0';
    }
  }
  return max_level;
}

// A decoded block candidate as the walk meets it (:1440-1450, 1647, 1663): 0 if it joins the chain, else the error.
int bz_block_verdict(const BlockOut& bo, uint32_t dbuf_size, uint64_t bitpos, bool timing) {
  if (timing) fprintf(stderr, "[cjs dec] block at bit %llu: err %d count %u orig %u crc %08x end %llu\n", (unsigned long long)bitpos, bo.err, bo.count, bo.orig, bo.crc, (unsigned long long)bo.end_bit);
  if (bo.err != CJS_E_OBSOLETE_INPUT && bo.orig > dbuf_size) { set_detail("initial position out of bounds"); return CJS_E_DATA_ERROR; }   // :1449-1450
  if (bo.err) return bo.err;
  if (bo.count > dbuf_size) return CJS_E_DATA_ERROR;             // decoded with the largest level's limit: this stream's is lower (:1647,1663)
  return 0;
}

// The chain walk of one input (Bunzip.decode :1776-1794): 32 -> end(block 0) -> end(block 1) ... over the candidates, stream CRC
// fold, multistream restarts (each member keeps its own level, :1787-1792).  in / n: the input's own bytes, whose header
// _start_bunzip has passed; positions are bits of the input.  `in` is anything indexable by byte: the host bytes, or (device
// source) an accessor over the few bytes the walk reads -- the header, and at an end-of-stream candidate the stored stream CRC and
// the restart header behind it.  at(pos, &kind, &bo) finds the candidate whose magic starts at bit
// pos (false: none) with its decode result, end_bit in bits of the input; take(bo, pos) appends a good block to the chain.
// Returns 0 or the first error the walk meets, its detail set.  mode 1 (Bunzip.table) does not test the stream CRC.
//
// `st` (a streaming decoder's step; nullptr: a walk of the whole input from its header on) holds the state the walk starts from
// and is left with the state it stopped in.  With st->partial the n bytes are only the stream so far, and the walk stops
// (st->stop != WALK_RUNS, return 0) in front of anything whose verdict the bytes still to come could change; with a row limit
// (st->cut_bit) it stops at the first candidate that was not decoded.  The state is that of the point where the walk stands:
// a later call with more bytes goes on from it.  take() sees *st as it was in front of the block it is given.
enum { WALK_RUNS = 0, WALK_ENDED, WALK_NEED_MAGIC, WALK_NEED_CRC, WALK_NEED_HEADER, WALK_NO_ROW, WALK_BLOCK_OPEN, WALK_ERR_NEAR_END, WALK_OUT_BUDGET };
struct WalkState {
  uint64_t pos = 32; uint32_t crc = 0, dbuf_size = 0;            // dbuf_size 0: from the input's header byte
  bool partial = false;
  uint64_t cut_bit = ~0ull, extent = 0;                          // extent: bytes a block can span (partial)
  int stop = WALK_RUNS;
};
template <typename Bytes, typename At, typename Take>
int bz_walk(const Bytes& in, size_t n, int multistream, int mode, uint32_t tt_stride, bool timing, At at, Take take, WalkState* st = nullptr) {
  auto read_bits = [&](uint64_t bit, int k) -> uint64_t { uint64_t v = 0; for (int i = 0; i < k; i++) { const uint64_t b = bit + i; v = (v << 1) | ((b >> 3) < n ? (in[b >> 3] >> (7 - (b & 7))) & 1u : 0u); } return v; };
  WalkState whole;
  if (!st) st = &whole;
  const bool partial = st->partial;
  uint32_t& dbuf_size = st->dbuf_size;                            // of the member stream being walked
  if (!dbuf_size) dbuf_size = 100000u * (uint32_t)(in[3] - '0');
  uint64_t& pos = st->pos; uint32_t& stream_crc = st->crc;
  auto stop = [&](int why) { st->stop = why; return 0; };
  for (;;) {
    if (partial ? pos + 48 > (uint64_t)n * 8 : (pos + 7) / 8 >= n) return stop(partial ? WALK_NEED_MAGIC : WALK_ENDED);      // inputStream.eof() (:1777)
    if (pos >= st->cut_bit) return stop(WALK_NO_ROW);
    uint32_t kind = 0; BlockOut bo;
    if (!at(pos, &kind, &bo)) return CJS_E_NOT_BZIP_DATA;        // h !== WHOLEPI (:1438)
    if (kind == 0) {
      const int rc = bz_block_verdict(bo, dbuf_size, pos, timing);
      // (partial) an error found less than a block's extent before the end may come from the zeros read past it; a good block
      // read nothing behind its end-of-block code, unless that was cut off (end_bit is clamped to the end)
      if (partial && rc && (pos >> 3) + st->extent > n) { clear_detail(); return stop(WALK_ERR_NEAR_END); }
      if (rc) return rc;
      if (partial && bo.end_bit >= (uint64_t)n * 8) return stop(WALK_BLOCK_OPEN);
      take(bo, pos);
      stream_crc = bo.crc ^ ((stream_crc << 1) | (stream_crc >> 31));
      pos = bo.end_bit;
    } else {
      if (partial && (pos + 80 > (uint64_t)n * 8 || (multistream && (pos + 80 + 7) / 8 + 4 > n))) return stop(pos + 80 > (uint64_t)n * 8 ? WALK_NEED_CRC : WALK_NEED_HEADER);
      const uint32_t target = (uint32_t)read_bits(pos + 48, 32);
      pos += 80;
      if ((pos + 7) / 8 > n) pos = (uint64_t)n * 8;
      if (timing) fprintf(stderr, "[cjs dec] end of stream at bit %llu: stream crc %08x stored %08x\n", (unsigned long long)pos - 80, stream_crc, target);
      if (mode == 0 && target != stream_crc) {                   // Bunzip.table ignores the stream crc (:1852)
        set_detail("Bad stream CRC (got %x expected %x)", stream_crc, target);
        return CJS_E_DATA_ERROR;
      }
      const uint64_t byte = (pos + 7) / 8;
      if (!multistream || byte >= n) return stop(WALK_ENDED);
      // _start_bunzip again, byte aligned (:1787-1792)
      uint8_t h[4] = {0, 0, 0, 0};
      for (uint64_t i = 0; i < 4 && byte + i < n; i++) h[i] = in[byte + i];
      int lv = 0; const char* why = nullptr;
      if (bz_header_check(h, (size_t)(n - byte), &lv, &why)) { set_detail("%s", why); return CJS_E_NOT_BZIP_DATA; }
      dbuf_size = 100000u * (uint32_t)lv;
      if (dbuf_size > tt_stride) return CJS_E_UNSUPPORTED;      // cannot happen: the pre-scan saw this header
      pos = (byte + 4) * 8; stream_crc = 0;
    }
  }
}

// The candidates a walk runs over: the sorted bits of one share's candidates, or of all the shares of a single-stream call in
// share order (their byte ranges ascend), each with its share and its index there.  base: the bit of the upload at which the
// input being walked starts (a batch group: 8 x bst[i]), so that find() takes the walk's own positions.
struct WalkCands {
  const DecShare* sh;
  std::vector<uint64_t> bit; std::vector<uint32_t> share, local;
  uint64_t base = 0;
  WalkCands(const DecShare* shares, size_t nsh) : sh(shares) {
    for (size_t i = 0; i < nsh; i++)
      for (size_t k = 0; k < sh[i].cands.size(); k++) { bit.push_back(sh[i].cands[k].bit); share.push_back((uint32_t)i); local.push_back((uint32_t)k); }
  }
  long find(uint64_t pos) const {
    const auto it = std::lower_bound(bit.begin(), bit.end(), base + pos);
    return (it != bit.end() && *it == base + pos) ? (long)(it - bit.begin()) : -1;
  }
  uint32_t kind(long ci) const { return sh[share[(size_t)ci]].cands[local[(size_t)ci]].kind; }
  const BlockOut& bo(long ci) const { return sh[share[(size_t)ci]].bos[local[(size_t)ci]]; }
  IbBlock chain_block(long ci) const {
    const BlockOut& b = bo(ci);
    IbBlock ib; ib.tt = sh[share[(size_t)ci]].tt_ptr[local[(size_t)ci]]; ib.count = b.count; ib.orig = b.orig; ib.off = 0; ib.woff = 0; ib.out_off = 0; ib.out_len = 0; ib.crc = b.crc;
    return ib;
  }
};

// bz_walk over C, the good blocks appended to J.chain.  met(ci, pos) is called for every candidate the walk accepts: an
// end-of-stream candidate when the walk finds it, before it reads the record behind the magic; a block once it is on the chain
// (a resumed walk's *st is then still the state in front of the block).
template <typename Bytes, typename Met>
int walk_chain(DecJob& J, const WalkCands& C, const Bytes& in, size_t n, int multistream, int mode, Met met, WalkState* st = nullptr) {
  long last = -1;
  return bz_walk(in, n, multistream, mode, J.tt_stride, J.timing,
                 [&](uint64_t pos, uint32_t* kind, BlockOut* bo) {
                   if ((last = C.find(pos)) < 0) return false;
                   *kind = C.kind(last); *bo = C.bo(last); bo->end_bit -= C.base;
                   if (*kind) met(last, pos);
                   return true;
                 },
                 [&](const BlockOut&, uint64_t pos) { J.chain.push_back(C.chain_block(last)); met(last, pos); }, st);
}
inline void met_nothing(long, uint64_t) {}

// exclusive prefix sum of the chain's decoded lengths (phase B's) -> J.out_off; returns the total
uint64_t chain_out_offsets(DecJob& J) {
  const size_t nb = J.chain.size();
  J.out_off.assign(nb + 1, 0);
  for (size_t k = 0; k < nb; k++) J.out_off[k + 1] = J.out_off[k] + J.chain[k].out_len;
  return J.out_off[nb];
}

}  // namespace

static int bunzip_core(const uint8_t* in, size_t n, int multistream, int mode, uint64_t at_bit, uint8_t** out, size_t* out_n,
                       uint64_t* tab_pos, uint32_t* tab_size, long tab_cap, long* tab_n, const cjs_opts* opts,
                       std::vector<cjs_bz_index_entry>* tab_ix = nullptr) {      // (mode 1: an index entry per block as well)
  if (out) *out = nullptr;
  if (out_n) *out_n = 0;
  if (tab_n) *tab_n = 0;
  clear_detail();
  CJS_TRY(select_device(opts));
  int level = 0; const char* why = nullptr;
  if (bz_header_check(in, n, &level, &why)) { set_detail("%s", why); return CJS_E_NOT_BZIP_DATA; }
  int ndev = 0, dev0 = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev0) != hipSuccess) return CJS_E_NO_DEVICE;

  DecJob J; J.in = in; J.n = n; J.mode = mode;
  J.timing = env_debug();
  J.tt_stride = 100000u * (uint32_t)bz_max_level(in, n, level, multistream && mode != 2);

  // shares: contiguous byte ranges, one per requested device slot
  uint32_t nsh = Opts(opts).n_devices;
  if (nsh < 1 || mode == 2) nsh = 1;
  if (nsh > 64) nsh = 64;
  if ((size_t)nsh * 65536 > n) nsh = (uint32_t)(n / 65536 ? n / 65536 : 1);     // tiny inputs: one share
  const uint64_t overlap = dec_extent(J.tt_stride);
  RestoreDevice restore{dev0};                                                  // after the shares have been released
  std::vector<DecShare> sh(nsh);
  for (uint32_t i = 0; i < nsh; i++) {
    DecShare& S = sh[i];
    S.device = nsh == 1 ? dev0 : (int)(i % (uint32_t)ndev);
    S.lo = (uint64_t)n * i / nsh; S.hi = (uint64_t)n * (i + 1) / nsh;
    S.up_lo = S.lo & ~(uint64_t)255;
    S.up_hi = std::min<uint64_t>(n, S.hi + overlap);
  }
  if (mode == 2) {                                                             // one block: upload from its byte on
    sh[0].lo = std::min<uint64_t>(at_bit >> 3, n); sh[0].hi = std::min<uint64_t>(n, sh[0].lo + 1);
    sh[0].up_lo = sh[0].lo & ~(uint64_t)255; sh[0].up_hi = std::min<uint64_t>(n, sh[0].hi + overlap);
  }
  const auto T0 = std::chrono::steady_clock::now();
  int rc = for_each_share(sh, &J, dec_phase_a);
  if (rc) return rc;
  const double ms_a = ms_since(T0);

  // ---- chain walk over all shares' candidates (Bunzip.decode :1776-1794)
  const WalkCands C(sh.data(), nsh);
  std::vector<uint32_t> chain_share;
  WalkState wst;                                                 // (a whole walk from the header on; met reads the member's level of it)
  auto met = [&](long ci, uint64_t pos) {
    if (C.kind(ci) != 0) return;
    J.chain_bits.push_back(pos); chain_share.push_back(C.share[(size_t)ci]);
    if (tab_ix) tab_ix->push_back(cjs_bz_index_entry{pos, C.bo(ci).end_bit, 0u, C.bo(ci).crc, wst.dbuf_size / 100000u, 0u});
  };
  if (mode == 2) {                                               // reader.seekBit(pos); _get_next_block() (:1803-1805)
    const long ci = C.find(at_bit);
    if (ci < 0) rc = CJS_E_NOT_BZIP_DATA;
    else if (C.kind(ci) == 0) {
      rc = bz_block_verdict(C.bo(ci), 100000u * (uint32_t)level, at_bit, J.timing);
      if (!rc) { J.chain.push_back(C.chain_block(ci)); met(ci, at_bit); }
    }
  } else rc = walk_chain(J, C, in, n, multistream, mode, met, &wst);
  // The reference decodes block after block and checks every block's CRC before it reads on (:1756-1761), so an error met
  // by the walk (bad stream CRC, damaged later block, broken chain) is reported only if every block in front of it
  // passes its own CRC check: keep it pending and run the rest of the pipeline, without output, over the chain so far.
  const int pending_rc = rc;
  char pending_detail[192];
  snprintf(pending_detail, sizeof pending_detail, "%s", cjs_last_error_detail());
  clear_detail();
  rc = 0;
  const size_t nb = J.chain.size();
  if (nb == 0) {
    if (pending_rc) { set_detail("%s", pending_detail); return pending_rc; }
    if (out) { *out = (uint8_t*)malloc(1); if (!*out) return CJS_E_OUT_OF_MEMORY; }
    return 0;
  }
  {  // the chain is increasing in bit position, so every share owns one contiguous run of it
    size_t k = 0;
    for (uint32_t i = 0; i < nsh; i++) { sh[i].c0 = k; while (k < nb && chain_share[k] == i) k++; sh[i].c1 = k; }
    if (k != nb) return CJS_E_DATA_ERROR;      // a chain that runs backwards: corrupt input
  }
  const auto T1 = std::chrono::steady_clock::now();
  rc = for_each_share(sh, &J, dec_phase_b);
  if (rc) return rc;
  const double ms_b = ms_since(T1);
  const uint64_t total = chain_out_offsets(J);
  if (out && !pending_rc) { J.host = (uint8_t*)HostPool::take(total ? (size_t)total : 1); if (!J.host) return CJS_E_OUT_OF_MEMORY; }
  const auto T2 = std::chrono::steady_clock::now();
  rc = for_each_share(sh, &J, dec_phase_c);
  const double ms_c = ms_since(T2);
  for (auto& x : sh) x.release();                              // (the streams have drained before J.host can go back)
  if (J.timing) {
    fprintf(stderr, "[cjs dec] %u share(s): upload + magic scan + block decode %.2f ms, inverse BWT + RLE1 lengths %.2f ms, RLE1 + CRC + D2H %.2f ms\n", nsh, ms_a, ms_b, ms_c);
    for (uint32_t i = 0; i < nsh; i++) fprintf(stderr, "[cjs dec]   share %u (device %d): %zu candidates, blocks [%zu, %zu): %.2f / %.2f / %.2f ms\n", i, sh[i].device,
                                               sh[i].cands.size(), sh[i].c0, sh[i].c1, sh[i].ms_a, sh[i].ms_b, sh[i].ms_c);
  }
  if (rc) { HostPool::give(J.host); return rc; }
  if (pending_rc) { set_detail("%s", pending_detail); return pending_rc; }
  if (tab_n) {
    *tab_n = (long)nb;
    for (size_t k = 0; k < nb && (long)k < tab_cap; k++) { tab_pos[k] = J.chain_bits[k]; tab_size[k] = J.chain[k].out_len; }
    if (tab_ix) for (size_t k = 0; k < nb; k++) (*tab_ix)[k].size = J.chain[k].out_len;
  }
  if (out) { *out = J.host; *out_n = (size_t)total; }
  return 0;
}

extern "C" int cjs_bzip2_decompress(const uint8_t* in, size_t n, int multistream, uint8_t** out, size_t* out_n, const cjs_opts* opts) {
  if (!out || !out_n) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  return bunzip_core(in, n, multistream, 0, 0, out, out_n, nullptr, nullptr, 0, nullptr, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
extern "C" int cjs_bzip2_decompress_block(const uint8_t* in, size_t n, uint64_t bitpos, uint8_t** out, size_t* out_n, const cjs_opts* opts) {
  if (!out || !out_n) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  return bunzip_core(in, n, 0, 2, bitpos, out, out_n, nullptr, nullptr, 0, nullptr, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
extern "C" long cjs_bzip2_table(const uint8_t* in, size_t n, int multistream, uint64_t* bitpos, uint32_t* size, long cap, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  long nbk = 0;
  const int rc = bunzip_core(in, n, multistream, 1, 0, nullptr, nullptr, bitpos, size, cap, &nbk, opts);
  return rc ? (long)rc : nbk;
  CJS_GUARD_END((long)CJS_E_OUT_OF_MEMORY, (long)CJS_E_HIP)
}

// ---------------------------------------------------------------- batch group (host form: dec_batch_group, device form: dev_group_*)
// Inputs go in groups of up to BATCH_DEC_GROUP_BYTES, each group one upload with every input at a 4-byte-aligned offset and one
// share of phases A-C: one magic scan over the group (a candidate never straddles two inputs), block decode of all candidates
// with every read bounded by the candidate's own input, then the walk of each input over the candidates of its bytes, phase B
// over all chain blocks, phase C with a CRC verdict per block.  An input larger than a group goes through the single-stream
// path.  What the two forms share is here; where the bytes come from and where they go is theirs.  See DESIGN.md §6c.
namespace {

constexpr size_t BATCH_DEC_GROUP_BYTES = (size_t)256 << 20;

size_t dec_group_bytes() {
  static const size_t g = getenv("CJS_DEC_GROUP_BYTES") ? (size_t)strtoull(getenv("CJS_DEC_GROUP_BYTES"), nullptr, 10) : BATCH_DEC_GROUP_BYTES;   // (tests shrink it)
  return g && g <= ((size_t)1 << 30) ? g : BATCH_DEC_GROUP_BYTES;      // (group offsets are 32-bit)
}

// the group that starts at input k0 (n[k0] <= G): inputs [k0, k1) whose 4-byte-aligned sizes come to G at most
size_t dec_group_end(const size_t* n, size_t count, size_t k0, size_t G) {
  size_t k1 = k0, bytes = 0;
  while (k1 < count && n[k1] <= G && (k1 == k0 || bytes + n[k1] <= G)) bytes += (n[k1++] + 3) & ~(size_t)3;
  return k1;
}

struct BatchGroup {
  size_t k0 = 0, k1 = 0;              // inputs [k0, k1) of the call
  std::vector<uint8_t> ok;            // input k0 + i passed _start_bunzip
  std::vector<size_t> ch0, ch1;       // input k0 + i's chain blocks
};

// The layout of a group: _start_bunzip (:1408-1427) of every input, the accepted ones at 4-byte-aligned offsets of one upload
// (S.bst / S.ben), each with the block size of its own single call (S.bdsz: the kernels' limits for its blocks), the rows sized
// for the largest of them.  hdr(k): the first bytes of input k; level(k, lv): its largest member level, lv being its header's;
// placed(k, at): input k lies at byte `at` of the upload.
template <typename Hdr, typename Level, typename Placed>
void group_layout(DecJob& J, DecShare& S, BatchGroup& G, size_t k0, size_t k1, const size_t* n, int32_t* status, std::vector<std::string>& detail,
                  Hdr hdr, Level level, Placed placed) {
  const size_t items = k1 - k0;
  G.k0 = k0; G.k1 = k1; G.ok.assign(items, 0);
  J.mode = 0; J.batch = true; J.timing = env_debug();
  S.bst.resize(items); S.ben.resize(items); S.bdsz.assign(items, 100000u);
  int max_level = 1;
  size_t bytes = 0;
  for (size_t i = 0; i < items; i++) {
    const size_t k = k0 + i;
    S.bst[i] = S.ben[i] = (uint32_t)bytes;
    int lv = 0; const char* why = nullptr;
    if ((status[k] = bz_header_check(hdr(k), n[k], &lv, &why)) != 0) { detail[k] = why; continue; }
    const int own = level(k, lv);
    S.bdsz[i] = 100000u * (uint32_t)own;
    max_level = std::max(max_level, own);
    G.ok[i] = 1;
    placed(k, bytes);
    S.ben[i] = (uint32_t)(bytes + n[k]);
    bytes = (bytes + n[k] + 3) & ~(size_t)3;
  }
  J.tt_stride = 100000u * (uint32_t)max_level;
  J.n = bytes;
  S.lo = 0; S.hi = bytes; S.up_lo = 0; S.up_hi = bytes;
}

// A laid-out group up to phase B: phase A over the upload, the walk of every accepted input over the candidates of its bytes
// (walk(k, C), C.base being the input's first bit of the upload; its error is pending: a bad block CRC in front of it wins),
// phase B over all chain blocks, the output offsets.  A failure of the call, or 0 and the bytes of the group's output.
template <typename Walk>
int group_prepare(DecJob& J, DecShare& S, BatchGroup& G, int32_t* status, std::vector<std::string>& detail, Walk walk, uint64_t* total) {
  if (J.n) {
    guarded(S.rc, [&] { dec_phase_a(&J, &S); });
    if (S.rc) return S.rc;
  }
  WalkCands C(&S, 1);
  const size_t items = G.k1 - G.k0;
  G.ch0.assign(items, 0); G.ch1.assign(items, 0);
  for (size_t i = 0; i < items; i++) {
    G.ch0[i] = G.ch1[i] = J.chain.size();
    if (!G.ok[i]) continue;
    C.base = 8ull * S.bst[i];
    clear_detail();
    const int rc = walk(G.k0 + i, C);
    G.ch1[i] = J.chain.size();
    if (rc) { status[G.k0 + i] = rc; detail[G.k0 + i] = cjs_last_error_detail(); }
  }
  clear_detail();
  S.c0 = 0; S.c1 = J.chain.size();
  if (S.c1) {
    guarded(S.rc, [&] { dec_phase_b(&J, &S); });
    // (phase B's own CJS_E_UNSUPPORTED / CJS_E_DATA_ERROR exits cannot happen -- a block holds <= 900000 bytes, a walk makes a step;
    // should one, it is a failure of the call, reported as one of the call's codes)
    if (S.rc == CJS_E_OUT_OF_MEMORY || S.rc == CJS_E_NO_DEVICE) return S.rc;
    if (S.rc) return CJS_E_HIP;
  }
  *total = chain_out_offsets(J);
  return 0;
}

// After phase C (J.crc_got): input k's verdict is the single call's -- the first block of its chain, in stream order, whose CRC
// fails (:1756-1761); else what its header or its walk left in status / detail; else success -- and its bytes: off from `base`
// on, len 0 for a failed input.
void group_verdicts(const DecJob& J, const BatchGroup& G, size_t base, size_t* off, size_t* len, int32_t* status, std::vector<std::string>& detail) {
  for (size_t i = 0; i < G.k1 - G.k0; i++) {
    const size_t k = G.k0 + i;
    for (size_t b = G.ch0[i]; b < G.ch1[i]; b++) if (J.crc_got[b] != J.chain[b].crc) {
      char d[96];
      bad_crc_detail(d, sizeof d, J.crc_got[b], J.chain[b].crc);
      status[k] = CJS_E_DATA_ERROR; detail[k] = d;
      break;
    }
    off[k] = base + (size_t)J.out_off[G.ch0[i]];
    len[k] = status[k] ? 0 : (size_t)(J.out_off[G.ch1[i]] - J.out_off[G.ch0[i]]);
  }
}

}  // namespace

// ---------------------------------------------------------------- device-resident source and sink (cjs_bzip2_decompress_device)
// bunzip_core with the input and the output in the GPU's memory.  The host path reads its host copy of the input in four places;
// each is a device pass here (dec_device.hip): the header (dd_headers, one 8-byte D2H), the level pre-scan of a multistream input
// (dd_level_scan: bz_max_level's rule), the upload (a device-to-device copy into phase A's dword-phased scratch) and, after the
// magic scan, the stored stream CRC and restart header of every end-of-stream candidate (dd_eos_bytes), which bz_walk reads
// through DevWalkBytes.  Phase C expands into the caller's buffer at the final offsets.  One share: the input lives on one GPU.
// See DESIGN.md §6d.
namespace {

bool on_device(const void* p, int dev) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice && a.device == dev;
}

// what bz_walk reads of a device input: its 4 header bytes, and EOS_REC bytes from byte `at` on at the end-of-stream candidate
// the walk stands on
struct DevWalkBytes {
  const uint8_t* hdr; const uint8_t* rec = nullptr; uint64_t at = 0;
  uint8_t operator[](uint64_t i) const { if (rec && i - at < (uint64_t)EOS_REC) return rec[i - at]; return i < 4 ? hdr[i] : (uint8_t)0; }
};

// J->eos of a device source: EOS_REC bytes per end-of-stream candidate (rec_of[c]: its record, -1 for a block candidate)
int dev_eos_gather(DecShare* S, std::vector<uint8_t>& rec, std::vector<long>& rec_of) {
  const size_t nc = S->cands.size();
  std::vector<uint64_t> tab;
  rec_of.assign(nc, -1);
  for (size_t c = 0; c < nc; c++) if (S->cands[c].kind) {
    rec_of[c] = (long)(tab.size() / 2);
    tab.push_back((S->cands[c].bit + 48) >> 3);
    tab.push_back(S->bst.empty() ? S->up_hi : S->ben[S->cands[c].pad]);      // (a batch candidate: its own input's end)
  }
  const uint32_t ne = (uint32_t)(tab.size() / 2);
  rec.assign((size_t)ne * EOS_REC, 0);
  if (!ne) return 0;
  uint64_t* d_tab = nullptr; uint8_t* d_rec = nullptr;
  ShareScratch q(S);
  CJS_TRY(q.take((void**)&d_tab, 16 * (size_t)ne));
  CJS_TRY(q.take((void**)&d_rec, (size_t)ne * EOS_REC));
  if (hipMemcpyAsync(d_tab, tab.data(), 16 * (size_t)ne, hipMemcpyHostToDevice, S->s) != hipSuccess) return CJS_E_HIP;
  launch_dev_eos_bytes(S->s, S->d_in, d_tab, ne, d_rec);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(rec.data(), d_rec, (size_t)ne * EOS_REC, hipMemcpyDeviceToHost, S->s) != hipSuccess ||
      hipStreamSynchronize(S->s) != hipSuccess) return CJS_E_HIP;
  S->h2d += 16 * (size_t)ne; S->d2h += (size_t)ne * EOS_REC;
  q.done();
  return 0;
}

// One decode of a device-resident source: a single stream (bunzip_core with one share) or a batch group (dec_batch_group).
// Prepared up to phase B, so that every size is known before anything is written, then emitted (phase C into the caller's buffer).
struct DevUnit {
  DecJob J;
  DecShare S;
  std::vector<uint8_t> rec; std::vector<long> rec_of;      // the end-of-stream candidates' bytes (dev_eos_gather)
  int pending = 0; char pending_detail[192] = {0};         // single: the walk's error, reported if every block in front passes its CRC
  uint64_t total = 0;                                       // bytes of the unit's output
  BatchGroup G;                                             // batch: inputs [G.k0, G.k1) of the call (a single stream of its own: one)
  std::vector<GatherPiece> pieces;                          // batch group: the gather of the inputs into the group layout
};

// _start_bunzip's bytes of `count` inputs (input k = d_in[off[k] .. off[k+1])), and for a multistream call the largest member level
// of each (bz_max_level), on S's stream and from its pool
int dev_headers(DecShare& S, const uint8_t* d_in, const std::vector<uint64_t>& off, bool multistream, std::vector<DevHdr>& hd) {
  const size_t count = off.size() - 1;
  hd.assign(count, DevHdr{});
  if (off.back() == off.front()) return 0;                       // (no bytes at all: every header is empty)
  if (hipSetDevice(S.device) != hipSuccess || (!S.s && hipStreamCreate(S.s.put()) != hipSuccess)) return CJS_E_HIP;
  uint64_t* d_off = nullptr; DevHdr* d_hdr = nullptr;
  ShareScratch q(&S);
  CJS_TRY(q.take((void**)&d_off, 8 * off.size()));
  CJS_TRY(q.take((void**)&d_hdr, sizeof(DevHdr) * count));
  if (hipMemcpyAsync(d_off, off.data(), 8 * off.size(), hipMemcpyHostToDevice, S.s) != hipSuccess) return CJS_E_HIP;
  launch_dev_headers(S.s, d_in, d_off, (uint32_t)count, multistream, off.front(), off.back(), d_hdr);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hd.data(), d_hdr, sizeof(DevHdr) * count, hipMemcpyDeviceToHost, S.s) != hipSuccess ||
      hipStreamSynchronize(S.s) != hipSuccess) return CJS_E_HIP;
  S.h2d += 8 * off.size(); S.d2h += sizeof(DevHdr) * count;
  q.done();
  return 0;
}

// the walk of one input over the candidates of its bytes (C.base: its first bit of the share's upload): the bytes behind an
// end-of-stream magic come from the candidate's record
int dev_walk(DevUnit& U, const WalkCands& C, const DevHdr& hd, size_t n, int multistream) {
  DevWalkBytes acc{hd.h};
  return walk_chain(U.J, C, acc, n, multistream, 0, [&](long ci, uint64_t pos) {
    if (C.kind(ci)) { acc.rec = U.rec.data() + (size_t)U.rec_of[(size_t)ci] * EOS_REC; acc.at = (pos + 48) >> 3; }
  });
}

// single stream, up to phase B: 0 (U.pending, U.total set) or what cjs_bzip2_decompress returns before its output stage
int dev_single_prepare(DevUnit& U, const uint8_t* d_in, size_t n, int multistream, const DevHdr& hd) {
  int level = 0; const char* why = nullptr;
  if (bz_header_check(hd.h, n, &level, &why)) { set_detail("%s", why); return CJS_E_NOT_BZIP_DATA; }
  DecJob& J = U.J; DecShare& S = U.S;
  J.n = n; J.mode = 0; J.timing = env_debug();
  J.tt_stride = 100000u * (uint32_t)(multistream ? std::max<int>(level, (int)hd.level) : level);
  J.upload = [d_in, n](DecShare* s, uint8_t* dst) { return hipMemcpyAsync(dst, d_in, n, hipMemcpyDeviceToDevice, s->s) != hipSuccess ? (int)CJS_E_HIP : 0; };
  J.eos = [&U](DecShare* s) { return dev_eos_gather(s, U.rec, U.rec_of); };
  S.lo = 0; S.hi = n; S.up_lo = 0; S.up_hi = n;
  guarded(S.rc, [&] { dec_phase_a(&J, &S); });
  if (S.rc) return S.rc;
  U.pending = dev_walk(U, WalkCands(&S, 1), hd, n, multistream);
  snprintf(U.pending_detail, sizeof U.pending_detail, "%s", cjs_last_error_detail());
  clear_detail();
  S.c0 = 0; S.c1 = J.chain.size();
  if (S.c1) {
    guarded(S.rc, [&] { dec_phase_b(&J, &S); });
    if (S.rc) return S.rc;
  }
  U.total = chain_out_offsets(J);
  return 0;
}

// single stream, phase C into d_out (nullptr: the CRC verdicts alone, in scratch; so with a pending error) -> the final verdict
int dev_single_emit(DevUnit& U, uint8_t* d_out) {
  if (!U.J.chain.empty()) {
    U.J.dev_out = U.pending ? nullptr : d_out; U.J.host = nullptr;
    U.S.rc = 0;
    guarded(U.S.rc, [&] { dec_phase_c(&U.J, &U.S); });
    if (U.S.rc) { if (U.S.detail[0]) set_detail("%s", U.S.detail); return U.S.rc; }
  }
  if (U.pending) { set_detail("%s", U.pending_detail); return U.pending; }
  return 0;
}

// a batch group up to phase B: the inputs (n[k] bytes from d_in + in_off[k] on, their headers in hd) are gathered into the group
// layout on the device, and a walk reads its bytes from hd and the end-of-stream records
int dev_group_prepare(DevUnit& U, const uint8_t* d_in, const size_t* in_off, const size_t* n, size_t k0, size_t k1, int multistream, const std::vector<DevHdr>& hd,
                      int32_t* status, std::vector<std::string>& detail) {
  DecJob& J = U.J;
  group_layout(J, U.S, U.G, k0, k1, n, status, detail, [&](size_t k) { return hd[k].h; },
               [&](size_t k, int level) { return multistream ? std::max<int>(level, (int)hd[k].level) : level; },
               [&](size_t k, size_t at) {
                 for (size_t p = 0; p < n[k]; p += GATHER_PIECE)      // (pieces of whole words: the last one of an input is zero-filled to one)
                   U.pieces.push_back(GatherPiece{in_off[k] + p, (uint32_t)(at + p), (uint32_t)std::min<size_t>(GATHER_PIECE, n[k] - p)});
               });
  J.upload = [&U, d_in](DecShare* s, uint8_t* dst) {
    GatherPiece* d_pc = nullptr;
    CJS_TRY(s->take((void**)&d_pc, sizeof(GatherPiece) * U.pieces.size()));
    if (hipMemcpyAsync(d_pc, U.pieces.data(), sizeof(GatherPiece) * U.pieces.size(), hipMemcpyHostToDevice, s->s) != hipSuccess) return (int)CJS_E_HIP;
    s->h2d += sizeof(GatherPiece) * U.pieces.size();
    launch_dev_gather(s->s, d_in, d_pc, (uint32_t)U.pieces.size(), dst);
    return hipGetLastError() != hipSuccess ? (int)CJS_E_HIP : 0;
  };
  J.eos = [&U](DecShare* s) { return dev_eos_gather(s, U.rec, U.rec_of); };
  return group_prepare(J, U.S, U.G, status, detail, [&](size_t k, const WalkCands& C) { return dev_walk(U, C, hd[k], n[k], multistream); }, &U.total);
}

// a batch group, phase C into d_out (the group's region): every input's status, offset (from d_out) and length
int dev_group_emit(DevUnit& U, uint8_t* d_out, size_t base, size_t* out_off, size_t* out_len, int32_t* status, std::vector<std::string>& detail) {
  DecJob& J = U.J;
  J.crc_got.assign(J.chain.size(), 0);
  J.dev_out = d_out;
  if (!J.chain.empty()) { U.S.rc = 0; guarded(U.S.rc, [&] { dec_phase_c(&J, &U.S); }); }
  if (U.S.rc) return U.S.rc;
  group_verdicts(J, U.G, base, out_off, out_len, status, detail);
  return 0;
}

}  // namespace

extern "C" int cjs_bzip2_decompress_device(const uint8_t* d_in, size_t n, int multistream, uint8_t* d_out, size_t out_cap, size_t* out_n, const cjs_opts* opts) {
  if (!out_n || (!d_in && n) || (!d_out && out_cap)) return CJS_E_INVALID_ARG;
  *out_n = 0;
  clear_detail();
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  int ndev = 0, dev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CJS_E_NO_DEVICE;
  RestoreDevice restore{dev};
  if ((n && !on_device(d_in, dev)) || (out_cap && !on_device(d_out, dev))) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  DevUnit U;
  U.S.device = dev;
  std::vector<DevHdr> hd;
  CJS_TRY(dev_headers(U.S, d_in, {0, (uint64_t)n}, multistream != 0, hd));
  int rc = dev_single_prepare(U, d_in, n, multistream, hd[0]);
  if (!rc && !U.pending && U.total > out_cap) { *out_n = (size_t)U.total; rc = CJS_E_OUTPUT_TOO_SMALL; }      // (d_out untouched)
  else if (!rc) rc = dev_single_emit(U, d_out);
  U.S.release();
  if (U.J.timing)
    fprintf(stderr, "[cjs dec dev] single: %zu bytes in, %llu bytes out, H2D %llu D2H %llu candidates %zu blocks %zu\n", n, (unsigned long long)U.total,
            (unsigned long long)U.S.h2d, (unsigned long long)U.S.d2h, U.S.cands.size(), U.J.chain.size());
  if (!rc) *out_n = (size_t)U.total;
  return rc;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// ---------------------------------------------------------------- recovery (cjs_bzip2_recover[_device])
// Phases A, B and C without the chain walk: one share over the whole input with rows sized for level 9 and no header check; every
// decodable block candidate becomes a "chain" block of phases B and C, which return a CRC verdict per block (DecJob::batch); the
// host then picks the survivors in ascending order (the rule: include/cjs_hip.h).  Phases B and C run over one inverse-BWT batch
// of the candidates at a time (dec_next_batch), phase C expanding into scratch of the batch's size, and only the survivors leave
// it: so the memory held is phase A's (the upload and the decoded rows, as for decompression) plus one batch's, however many
// candidates there are.  The stream form gathers the survivors' bit strings from the upload, which stays with the share, into a
// zeroed buffer of the new stream's size (bz_bits_gather).  See DESIGN.md §6g.
namespace cjs {

// Bits [src_bit, src_bit + nbits) of a source go to bits [dst_bit, ..) of `out`; bit b of either is bit 31 - (b & 31) of the
// big-endian 32-bit word b >> 5.  src: the device address of the source's word 0 (4-byte aligned), src_words: the words of it
// that may be read.  nbits >= 1.
struct BitRun { uint64_t src, src_words, src_bit, dst_bit, nbits; };
// One thread per DESTINATION word of a run (workgroups along grid.x stride over the run's words, grid.y = the runs of a slab):
// the two source words the word straddles, a funnel shift, and the mask of the destination bits that are the run's -- what lies
// in front of the first and behind the last source bit belongs to other blocks or to damage.  A word wholly inside its run is
// stored; the first and the last word of a run, which two runs may share, are ORed into the zeroed buffer.
__global__ __launch_bounds__(256) void bz_bits_gather(const BitRun* __restrict__ runs, uint32_t run0, uint32_t* __restrict__ out) {
  const BitRun r = runs[run0 + blockIdx.y];
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(r.src);
  const uint64_t d1 = r.dst_bit + r.nbits, w0 = r.dst_bit >> 5, w1 = (d1 - 1) >> 5;
  for (uint64_t w = w0 + (uint64_t)blockIdx.x * 256 + threadIdx.x; w <= w1; w += (uint64_t)gridDim.x * 256) {
    const int64_t t = (int64_t)r.src_bit + ((int64_t)(w << 5) - (int64_t)r.dst_bit);      // the source bit that lands on the word's first bit
    const int64_t wi = t >> 5;                                                              // (floor: t >= -31)
    const uint32_t sh = (uint32_t)(t & 31);
    const uint32_t hi = wi >= 0 && (uint64_t)wi < r.src_words ? __builtin_bswap32(src[wi]) : 0u;
    const uint32_t lo = sh && wi + 1 >= 0 && (uint64_t)(wi + 1) < r.src_words ? __builtin_bswap32(src[wi + 1]) : 0u;
    uint32_t v = sh ? __builtin_amdgcn_alignbit(hi, lo, 32u - sh) : hi;
    const uint32_t a = w == w0 ? (uint32_t)(r.dst_bit & 31) : 0u, b = w == w1 ? (uint32_t)((d1 - 1) & 31) + 1u : 32u;      // the run's bits [a, b) of the word
    const uint32_t mask = (0xFFFFFFFFu >> a) & (b == 32u ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> b));
    v = __builtin_bswap32(v & mask);
    if (mask == 0xFFFFFFFFu) out[w] = v; else atomicOr(&out[w], v);
  }
}

}  // namespace cjs

namespace {

// the recovered bytes on the host: a HostPool buffer that grows batch by batch (one batch -- the usual case -- never copies)
struct RecHost {
  uint8_t* p = nullptr; size_t cap = 0;
  ~RecHost() { HostPool::give(p); }
  int ensure(size_t used, size_t need) {
    if (need <= cap && p) return 0;
    const size_t nc = std::max<size_t>(std::max<size_t>(need, 2 * cap), 1);
    uint8_t* q = (uint8_t*)HostPool::take(nc);
    if (!q) return CJS_E_OUT_OF_MEMORY;
    if (used) memcpy(q, p, used);
    HostPool::give(p);
    p = q; cap = nc;
    return 0;
  }
  uint8_t* release() { uint8_t* q = p; p = nullptr; cap = 0; return q; }
};

// in: the input on the host, or nullptr with d_src: the input on device `dev`.  host_out: the host form's result; else d_out /
// out_cap (checked by the caller).  found / cap / n_found as in the C ABI.
int recover_core(const uint8_t* in, const uint8_t* d_src, size_t n, bool as_stream, uint8_t** host_out, uint8_t* d_out, size_t out_cap, size_t* out_n,
                 cjs_bz_found* found, long cap, long* n_found, int dev) {
  RecHost host;                                                   // (declared first: given back after the share's stream has drained)
  DecJob J; DecShare S;
  J.in = in; J.n = n; J.mode = 0; J.batch = true; J.timing = env_debug();
  J.tt_stride = 900000u;
  if (d_src) J.upload = [d_src, n](DecShare* s, uint8_t* dst) { return hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToDevice, s->s) != hipSuccess ? (int)CJS_E_HIP : 0; };
  S.device = dev; S.lo = 0; S.hi = n; S.up_lo = 0; S.up_hi = n;
  guarded(S.rc, [&] { dec_phase_a(&J, &S); });
  if (S.rc) return S.rc;
  hipStream_t s = S.s;
  // phase B gives a one-batch share's rows back when it ends: here it runs once per batch of candidates, the rows stay to the end
  uint8_t* rows = S.d_tt; S.d_tt = nullptr;

  std::vector<uint32_t> bc;                                       // the block candidates (indices into S.cands), ascending
  for (uint32_t c = 0; c < S.cands.size(); c++) if (S.cands[c].kind == 0) bc.push_back(c);
  const size_t nc = bc.size();
  *n_found = (long)nc;
  const uint64_t nbits = (uint64_t)n * 8;
  std::vector<uint32_t> chain_bc;                                 // chain block k is block candidate chain_bc[k]
  for (size_t i = 0; i < nc; i++) {
    const BlockOut& bo = S.bos[bc[i]];
    if (bo.err || bo.end_bit >= nbits) continue;                  // (the decoder clamps end_bit to the end: a block that touches it may have been cut off)
    IbBlock ib; ib.tt = S.tt_ptr[bc[i]]; ib.count = bo.count; ib.orig = bo.orig; ib.off = 0; ib.woff = 0; ib.out_off = 0; ib.out_len = 0; ib.crc = bo.crc;
    J.chain.push_back(ib); chain_bc.push_back((uint32_t)i);
  }
  const size_t nb = J.chain.size();
  J.crc_got.assign(nb, 0);
  J.out_off.assign(nb + 1, 0);

  std::vector<BitRun> runs;                                       // stream form: header, survivors, trailer
  uint64_t total = 0, last_end = 0, sbit = 32;                    // bytes recovered so far / the selection's state / the new stream's next bit
  uint32_t fold = 0;
  const uint64_t src_addr = (uint64_t)(uintptr_t)S.d_in, src_words = ((uint64_t)n + 3) / 4;      // (the upload has 256 bytes of slack)
  size_t next = 0;                                                // block candidates in front of `next` have their entry
  auto entry = [&](size_t i, int status, uint64_t end_bit, uint64_t off, uint32_t size) {
    if (!found || (long)i >= cap) return;
    cjs_bz_found& f = found[i];
    f.bitpos = S.cands[bc[i]].bit; f.end_bit = end_bit; f.out_off = off; f.size = size; f.status = status; f.crc = S.bos[bc[i]].crc; f.reserved = 0;
  };
  auto lost_upto = [&](size_t i1) {                               // the candidates that are not decodable, up to i1
    for (; next < i1; next++) {
      const BlockOut& bo = S.bos[bc[next]];
      entry(next, S.cands[bc[next]].bit < last_end ? CJS_REC_SHADOWED : bo.err ? bo.err : CJS_E_DATA_ERROR, 0, 0, 0);
    }
  };
  int rc = 0;
  for (size_t g0 = 0; g0 < nb && !rc;) {
    const size_t g1 = dec_next_batch(&J, g0, nb);
    S.c0 = g0; S.c1 = g1; S.rc = 0;
    guarded(S.rc, [&] { dec_phase_b(&J, &S); });
    if (S.rc) { rc = S.rc == CJS_E_OUT_OF_MEMORY || S.rc == CJS_E_NO_DEVICE ? S.rc : CJS_E_HIP; break; }      // (its other exits cannot happen: see group_prepare)
    J.out_off[g0] = 0;                                            // (offsets inside the batch's scratch)
    for (size_t k = g0; k < g1; k++) J.out_off[k + 1] = J.out_off[k] + J.chain[k].out_len;
    const uint64_t gbytes = J.out_off[g1];
    uint8_t* d_exp = nullptr;
    if ((rc = S.take((void**)&d_exp, (size_t)gbytes + 64)) != 0) break;
    J.dev_out = d_exp; J.host = nullptr;
    guarded(S.rc, [&] { dec_phase_c(&J, &S); });
    if (S.rc) { rc = S.rc; break; }
    // the selection over this batch, and the survivors' bytes as runs of neighbours in the scratch
    struct Piece { uint64_t from, to, len; };
    std::vector<Piece> pieces;
    for (size_t k = g0; k < g1; k++) {
      const size_t i = chain_bc[k];
      lost_upto(i);
      const uint64_t p = S.cands[bc[i]].bit, e = S.bos[bc[i]].end_bit;
      next = i + 1;
      if (p < last_end) { entry(i, CJS_REC_SHADOWED, e, 0, 0); continue; }
      if (J.crc_got[k] != J.chain[k].crc) { entry(i, CJS_E_DATA_ERROR, e, 0, 0); continue; }
      const uint32_t len = J.chain[k].out_len;
      entry(i, 0, e, as_stream ? sbit : total, len);
      last_end = e;
      if (as_stream) {
        runs.push_back(BitRun{src_addr, src_words, p, sbit, e - p});
        sbit += e - p;
        fold = ((fold << 1) | (fold >> 31)) ^ J.chain[k].crc;
      } else if (len) {
        if (!pieces.empty() && pieces.back().from + pieces.back().len == J.out_off[k]) pieces.back().len += len;
        else pieces.push_back(Piece{J.out_off[k], total, len});
      }
      total += len;
    }
    if (!as_stream && !pieces.empty()) {
      if (host_out && (rc = host.ensure((size_t)pieces[0].to, (size_t)total)) != 0) break;
      for (const Piece& q : pieces) {
        hipError_t e = hipSuccess;
        if (host_out) e = hipMemcpyAsync(host.p + q.to, d_exp + q.from, (size_t)q.len, hipMemcpyDeviceToHost, s);
        else if (q.to + q.len <= out_cap) e = hipMemcpyAsync(d_out + q.to, d_exp + q.from, (size_t)q.len, hipMemcpyDeviceToDevice, s);      // (what does not fit is only counted)
        if (e != hipSuccess) { rc = CJS_E_HIP; break; }
        if (host_out) S.d2h += q.len;
      }
      if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = CJS_E_HIP;
      if (rc) break;
    }
    S.drop(d_exp); S.drop(S.d_w); S.drop(S.d_carry);              // (the stream has drained)
    S.d_w = nullptr; S.d_carry = nullptr;
    g0 = g1;
  }
  if (rc) return rc;
  lost_upto(nc);
  if (rows) S.drop(rows);

  if (as_stream) {
    // header and trailer are two more runs, from a 16-byte source of their own: 'BZh9', then the end magic and the combined CRC
    uint8_t ht[16] = {'B', 'Z', 'h', '9', 0x17, 0x72, 0x45, 0x38, 0x50, 0x90, (uint8_t)(fold >> 24), (uint8_t)(fold >> 16), (uint8_t)(fold >> 8), (uint8_t)fold, 0, 0};
    const uint64_t sbits = sbit + 80;
    total = (sbits + 7) / 8;
    const size_t words = (size_t)((sbits + 31) / 32);
    uint8_t* d_ht = nullptr; BitRun* d_runs = nullptr; uint32_t* d_str = nullptr;
    CJS_TRY(S.take((void**)&d_ht, 16));
    runs.push_back(BitRun{(uint64_t)(uintptr_t)d_ht, 4, 0, 0, 32});
    runs.push_back(BitRun{(uint64_t)(uintptr_t)d_ht, 4, 32, sbit, 80});
    CJS_TRY(S.take((void**)&d_runs, sizeof(BitRun) * runs.size()));
    CJS_TRY(S.take((void**)&d_str, 4 * words));
    if (hipMemcpyAsync(d_ht, ht, 16, hipMemcpyHostToDevice, s) != hipSuccess || hipMemcpyAsync(d_runs, runs.data(), sizeof(BitRun) * runs.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(d_str, 0, 4 * words, s) != hipSuccess) return CJS_E_HIP;
    S.h2d += 16 + sizeof(BitRun) * runs.size();
    for (size_t r0 = 0; r0 < runs.size(); r0 += 65535) {          // (grid.y)
      const uint32_t nr = (uint32_t)std::min<size_t>(65535, runs.size() - r0);
      uint64_t mx = 0;
      for (size_t r = r0; r < r0 + nr; r++) mx = std::max(mx, runs[r].nbits);
      const uint32_t gx = (uint32_t)std::min<uint64_t>(256, (mx / 32 + 2 + 255) / 256);
      hipLaunchKernelGGL(bz_bits_gather, dim3(gx, nr), dim3(256), 0, s, d_runs, (uint32_t)r0, d_str);
    }
    if (hipGetLastError() != hipSuccess) return CJS_E_HIP;
    hipError_t e = hipSuccess;
    if (host_out) {
      CJS_TRY(host.ensure(0, (size_t)total));
      e = hipMemcpyAsync(host.p, d_str, (size_t)total, hipMemcpyDeviceToHost, s);
      S.d2h += total;
    } else if (total <= out_cap) e = hipMemcpyAsync(d_out, d_str, (size_t)total, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return CJS_E_HIP;
  }
  S.release();
  if (J.timing)
    fprintf(stderr, "[cjs recover] %zu bytes in, %zu candidates, %zu decodable, %u row batches (phase A), %u inverse-BWT batches, %llu bytes out (%s), H2D %llu D2H %llu\n", n, nc, nb,
            S.a_batches, S.b_batches, (unsigned long long)total, as_stream ? "stream" : "bytes", (unsigned long long)S.h2d, (unsigned long long)S.d2h);
  *out_n = (size_t)total;
  if (host_out) {
    CJS_TRY(host.ensure(0, 1));                                  // (nothing recovered: still a buffer, as cjs_bzip2_decompress gives)
    *host_out = host.release();
    return 0;
  }
  return total > out_cap ? (int)CJS_E_OUTPUT_TOO_SMALL : 0;
}

// the stream form of "nothing found" (n < 6: no device needed)
const uint8_t REC_EMPTY_STREAM[14] = {'B', 'Z', 'h', '9', 0x17, 0x72, 0x45, 0x38, 0x50, 0x90, 0, 0, 0, 0};

}  // namespace

extern "C" int cjs_bzip2_recover(const uint8_t* in, size_t n, int as_stream, uint8_t** out, size_t* out_n, cjs_bz_found* found, long cap, long* n_found,
                                 const cjs_opts* opts) {
  if (!out || !out_n || !n_found || (!in && n) || (!found && cap > 0)) return CJS_E_INVALID_ARG;
  *out = nullptr; *out_n = 0; *n_found = 0;
  clear_detail();
  CJS_GUARD_BEGIN
  if (n < 6) {
    const size_t sz = as_stream ? sizeof REC_EMPTY_STREAM : 0;
    if (!(*out = (uint8_t*)malloc(sz ? sz : 1))) return CJS_E_OUT_OF_MEMORY;
    if (sz) memcpy(*out, REC_EMPTY_STREAM, sz);
    *out_n = sz;
    return 0;
  }
  CJS_TRY(select_device(opts));
  int ndev = 0, dev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CJS_E_NO_DEVICE;
  RestoreDevice restore{dev};
  const int rc = recover_core(in, nullptr, n, as_stream != 0, out, nullptr, 0, out_n, found, cap, n_found, dev);
  if (rc) { *out_n = 0; *n_found = 0; }
  return rc;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_recover_device(const uint8_t* d_in, size_t n, int as_stream, uint8_t* d_out, size_t out_cap, size_t* out_n, cjs_bz_found* found, long cap,
                                        long* n_found, const cjs_opts* opts) {
  if (!out_n || !n_found || (!d_in && n) || (!d_out && out_cap) || (!found && cap > 0)) return CJS_E_INVALID_ARG;
  *out_n = 0; *n_found = 0;
  clear_detail();
  CJS_GUARD_BEGIN
  if (n < 6 && !as_stream) return 0;
  CJS_TRY(select_device(opts));
  int ndev = 0, dev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CJS_E_NO_DEVICE;
  RestoreDevice restore{dev};
  if ((n && !on_device(d_in, dev)) || (out_cap && !on_device(d_out, dev))) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  if (n < 6) {                                                    // the empty stream
    *out_n = sizeof REC_EMPTY_STREAM;
    if (out_cap < sizeof REC_EMPTY_STREAM) return CJS_E_OUTPUT_TOO_SMALL;
    return hipMemcpy(d_out, REC_EMPTY_STREAM, sizeof REC_EMPTY_STREAM, hipMemcpyHostToDevice) != hipSuccess ? (int)CJS_E_HIP : 0;
  }
  const int rc = recover_core(nullptr, d_in, n, as_stream != 0, nullptr, d_out, out_cap, out_n, found, cap, n_found, dev);
  if (rc && rc != CJS_E_OUTPUT_TOO_SMALL) { *out_n = 0; *n_found = 0; }
  return rc;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// ---------------------------------------------------------------- indexed range reads (cjs_bzip2_read_ranges[_device])
// recover_core's shape with the candidates given by an index instead of found by the scan: the blocks that the ranges touch go
// through phases A, B and C in ascending passes, a pass being what one upload of the batch decoder's group size holds.  Only the
// byte runs of a pass's blocks are uploaded, packed (range_pass_upload), and phase A is told its candidates (DecJob::given): no
// magic scan, no stream header, no chain walk -- a block stands or falls by its own index entry.  Phase C expands a batch of
// blocks into scratch, where their CRCs are computed, and the slice gather (range.hip) takes every piece of every range from
// there to its place.  See DESIGN.md §6h.
namespace {

enum { RG_GOOD = 0, RG_MISMATCH = 1, RG_BAD_CRC = 2 };
struct RangePiece { uint32_t block, in_off, len, pad; uint64_t out; };      // len bytes from byte in_off of the block to byte `out` of the layout

// What the index alone says about a call: the layout (lay_off / lay_len: range k clipped, packed in range order), the pieces
// sorted by block and the touched blocks, ascending.
struct RangePlan {
  std::vector<uint64_t> lay_off, lay_len;
  std::vector<RangePiece> pieces;
  std::vector<uint32_t> touched;
  uint64_t total = 0;
  size_t first_block(const cjs_bz_index* ix, uint64_t o) const { return (size_t)(std::upper_bound(ix->off.begin(), ix->off.end(), o) - ix->off.begin()) - 1; }
};

int range_plan(const cjs_bz_index* ix, const uint64_t* off, const uint64_t* len, size_t count, RangePlan& P) {
  const uint64_t end = ix->off.back();
  P.lay_off.assign(count, 0); P.lay_len.assign(count, 0);
  for (size_t k = 0; k < count; k++) {
    if (off[k] + len[k] < off[k]) { set_detail("range %zu: offset + length overflows", k); return CJS_E_INVALID_ARG; }
    P.lay_off[k] = P.total;
    if (off[k] >= end || !len[k]) continue;
    P.lay_len[k] = std::min<uint64_t>(len[k], end - off[k]);
    uint64_t pos = off[k], left = P.lay_len[k];
    for (size_t b = P.first_block(ix, pos); left; b++) {
      const uint64_t take = std::min<uint64_t>(left, ix->off[b + 1] - pos);
      if (take) P.pieces.push_back(RangePiece{(uint32_t)b, (uint32_t)(pos - ix->off[b]), (uint32_t)take, 0u, P.total + (pos - off[k])});
      pos += take; left -= take;
    }
    P.total += P.lay_len[k];
  }
  std::stable_sort(P.pieces.begin(), P.pieces.end(), [](const RangePiece& a, const RangePiece& b) { return a.block < b.block; });
  for (const RangePiece& p : P.pieces) if (P.touched.empty() || P.touched.back() != p.block) P.touched.push_back(p.block);
  return 0;
}

// One pass's upload: the byte runs [bitpos >> 3, (end_bit + 7) >> 3) of touched blocks [t0, t1), neighbours merged, each run at a
// packed offset congruent to its source address mod 16 (the device gather then stores aligned vectors from aligned vectors).
struct RangeRun { uint64_t lo, hi, at; };      // stream bytes [lo, hi) at byte `at` of the upload
struct RangeUpload {
  std::vector<RangeRun> runs; std::vector<uint64_t> bit;      // bit[i]: where touched block t0 + i's magic starts in the upload
  uint64_t bytes = 0;
  uint64_t bytes_with(const cjs_bz_index_entry& e, uint64_t src_addr) const {      // `bytes` once e has been added
    const uint64_t lo = e.bitpos >> 3, hi = (e.end_bit + 7) >> 3;
    if (runs.empty() || lo > runs.back().hi) return ((bytes + 15) & ~15ull) + ((src_addr + lo) & 15u) + (hi - lo);
    return runs.back().at + (std::max(runs.back().hi, hi) - runs.back().lo);
  }
  void add(const cjs_bz_index_entry& e, uint64_t src_addr) {
    const uint64_t lo = e.bitpos >> 3, hi = (e.end_bit + 7) >> 3;
    if (runs.empty() || lo > runs.back().hi) {
      const uint64_t at = ((bytes + 15) & ~15ull) + ((src_addr + lo) & 15u);
      runs.push_back(RangeRun{lo, hi, at});
    } else runs.back().hi = std::max(runs.back().hi, hi);
    bytes = runs.back().at + (runs.back().hi - runs.back().lo);
    bit.push_back((runs.back().at - runs.back().lo) * 8 + e.bitpos);
  }
};

constexpr uint64_t RANGE_PASS_DECODED = 4ull << 30;      // decoded bytes of a pass by the index (what phase A keeps of it is at most 1.25 x that)

size_t range_pass_blocks() {      // (read at every call: tests run the several-pass path at small sizes)
  const char* v = getenv("CJS_RANGE_PASS_BLOCKS");
  const unsigned long long x = v ? strtoull(v, nullptr, 10) : 0;
  return x ? (size_t)x : ~(size_t)0;
}

// slices of one piece of `len` bytes, cut where the destination crosses a multiple of SLICE_TASK behind its first 16-byte boundary
void range_slices(std::vector<Slice>& sl, uint64_t src, uint64_t dst, uint64_t len) {
  uint64_t cut = std::min<uint64_t>(len, SLICE_TASK - (dst & 15u));
  for (uint64_t o = 0; o < len; cut = std::min<uint64_t>(len - o, SLICE_TASK)) { sl.push_back(Slice{src + o, dst + o, cut}); o += cut; }
}

struct RangeStats { uint64_t h2d = 0, d2h = 0, up = 0; uint32_t passes = 0, a_batches = 0, b_batches = 0; size_t slices = 0; };

// in: the stream on the host, or nullptr with d_src: the stream on device `dev`.  host_out: the host form's buffer in the plan's
// layout; else d_out.  verdict / crc_got: per block of the index (RG_*; the computed CRC of an RG_BAD_CRC block).
int range_run(const uint8_t* in, const uint8_t* d_src, const cjs_bz_index* ix, const RangePlan& P, uint8_t* host_out, uint8_t* d_out,
              std::vector<uint8_t>& verdict, std::vector<uint32_t>& crc_got, int dev, RangeStats& st) {
  const size_t nt = P.touched.size(), cap_blocks = range_pass_blocks(), G = dec_group_bytes();
  Stream keep;                                                     // one stream for all passes
  size_t piece_at = 0;                                             // pieces in front of it belong to earlier blocks
  for (size_t t0 = 0; t0 < nt;) {
    // ---- the pass: touched blocks [t0, t1)
    RangeUpload U;
    size_t t1 = t0; uint32_t max_level = 1; uint64_t decoded = 0;
    while (t1 < nt && t1 - t0 < cap_blocks && t1 - t0 < DEC_BATCH_BLOCKS) {
      const cjs_bz_index_entry& e = ix->e[P.touched[t1]];
      if (t1 > t0 && (U.bytes_with(e, (uint64_t)(uintptr_t)d_src) > G || decoded + e.size > RANGE_PASS_DECODED)) break;
      U.add(e, (uint64_t)(uintptr_t)d_src);
      max_level = std::max(max_level, e.level); decoded += e.size; t1++;
    }
    st.passes++; st.up += U.bytes;
    const uint64_t up_n = U.bytes;
    struct HostGive { void* p; ~HostGive() { HostPool::give(p); } } staged{nullptr};      // (declared in front of the share: given back once its stream has drained)
    DecJob J; DecShare S;
    S.s = std::move(keep);
    J.n = (size_t)up_n; J.mode = 0; J.batch = true; J.given = true; J.timing = false;
    J.tt_stride = 100000u * max_level;
    S.device = dev; S.lo = 0; S.hi = up_n; S.up_lo = 0; S.up_hi = up_n;
    std::vector<uint32_t> cand_of(t1 - t0, ~0u);                  // touched block t0 + i's candidate (~0: its magic is not there)
    if (in) {                                                      // host form: the runs staged in one buffer, the magics checked here
      if (!(staged.p = HostPool::take((size_t)up_n))) return CJS_E_OUT_OF_MEMORY;
      for (const RangeRun& r : U.runs) memcpy((uint8_t*)staged.p + r.at, in + r.lo, (size_t)(r.hi - r.lo));
      J.in = (const uint8_t*)staged.p;
      for (size_t i = 0; i < t1 - t0; i++) {
        const uint64_t bp = ix->e[P.touched[t0 + i]].bitpos;
        uint64_t w = 0;
        for (int q = 0; q < 7; q++) w = (w << 8) | in[(bp >> 3) + q];      // (end_bit > bitpos + 80 and end_bit <= 8 n: inside the stream)
        if (((w >> (8 - (bp & 7))) & 0xFFFFFFFFFFFFull) != MAGIC_BLOCK) continue;
        cand_of[i] = (uint32_t)S.cands.size();
        S.cands.push_back(Cand{U.bit[i], 0u, 0u});
      }
    } else {                                                       // device form: one gather launch, one magic-check launch
      for (size_t i = 0; i < t1 - t0; i++) { cand_of[i] = (uint32_t)i; S.cands.push_back(Cand{U.bit[i], 0u, 0u}); }
      J.upload = [&U, d_src](DecShare* s, uint8_t* dst) {
        std::vector<Slice> sl;
        for (const RangeRun& r : U.runs) range_slices(sl, (uint64_t)(uintptr_t)d_src + r.lo, (uint64_t)(uintptr_t)dst + r.at, r.hi - r.lo);
        Slice* d_sl = nullptr;
        CJS_TRY(s->take((void**)&d_sl, sizeof(Slice) * sl.size()));      // (stays with the share: the copy below may still read `sl` -- it is synchronous for pageable memory)
        if (hipMemcpy(d_sl, sl.data(), sizeof(Slice) * sl.size(), hipMemcpyHostToDevice) != hipSuccess) return (int)CJS_E_HIP;
        s->h2d += sizeof(Slice) * sl.size();
        launch_slices(s->s, d_sl, sl.size());
        return hipGetLastError() != hipSuccess ? (int)CJS_E_HIP : 0;
      };
      J.vet = [&cand_of](DecShare* s) {
        const uint32_t nc = (uint32_t)s->cands.size();
        std::vector<uint64_t> bits(nc); std::vector<uint32_t> ok(nc);
        for (uint32_t c = 0; c < nc; c++) bits[c] = s->cands[c].bit;
        uint64_t* d_bits = nullptr; uint32_t* d_ok = nullptr;
        ShareScratch q(s);
        CJS_TRY(q.take((void**)&d_bits, 8 * (size_t)nc));
        CJS_TRY(q.take((void**)&d_ok, 4 * (size_t)nc));
        if (hipMemcpy(d_bits, bits.data(), 8 * (size_t)nc, hipMemcpyHostToDevice) != hipSuccess) return (int)CJS_E_HIP;
        launch_cand_magic(s->s, s->d_in, s->up_hi, d_bits, nc, d_ok);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(ok.data(), d_ok, 4 * (size_t)nc, hipMemcpyDeviceToHost, s->s) != hipSuccess ||
            hipStreamSynchronize(s->s) != hipSuccess) return (int)CJS_E_HIP;
        s->h2d += 8 * (size_t)nc; s->d2h += 4 * (size_t)nc;
        std::vector<Cand> kept;                                      // (candidate c is touched block t0 + c until here)
        for (uint32_t c = 0; c < nc; c++) {
          cand_of[c] = ok[c] ? (uint32_t)kept.size() : ~0u;
          if (ok[c]) kept.push_back(s->cands[c]);
        }
        s->cands.swap(kept);
        q.done();
        return 0;
      };
    }
    if (!S.cands.empty()) {
      guarded(S.rc, [&] { dec_phase_a(&J, &S); });
      if (S.rc) return S.rc;
    }
    hipStream_t s = S.s;
    uint8_t* rows = S.d_tt; S.d_tt = nullptr;                      // (phase B runs once per batch here: see recover_core)

    // ---- the blocks that agree with their entries so far become the chain of phases B and C
    std::vector<uint32_t> chain_blk;
    for (size_t i = 0; i < t1 - t0; i++) {
      const uint32_t b = P.touched[t0 + i], c = cand_of[i];
      const cjs_bz_index_entry& e = ix->e[b];
      verdict[b] = RG_MISMATCH;
      if (c == ~0u || S.cands[c].kind != 0) continue;
      const BlockOut& bo = S.bos[c];
      const int v = bz_block_verdict(bo, 100000u * e.level, e.bitpos, false);
      clear_detail();
      if (v || !bo.count || bo.end_bit - (U.bit[i] - e.bitpos) != e.end_bit || bo.crc != e.crc) continue;
      IbBlock ib; ib.tt = S.tt_ptr[c]; ib.count = bo.count; ib.orig = bo.orig; ib.off = 0; ib.woff = 0; ib.out_off = 0; ib.out_len = 0; ib.crc = bo.crc;
      J.chain.push_back(ib); chain_blk.push_back(b);
    }
    const size_t nb = J.chain.size();
    J.crc_got.assign(nb, 0);
    J.out_off.assign(nb + 1, 0);
    int rc = 0;
    for (size_t g0 = 0; g0 < nb && !rc;) {
      const size_t g1 = dec_next_batch(&J, g0, nb);
      S.c0 = g0; S.c1 = g1; S.rc = 0;
      guarded(S.rc, [&] { dec_phase_b(&J, &S); });
      if (S.rc) { rc = S.rc == CJS_E_OUT_OF_MEMORY || S.rc == CJS_E_NO_DEVICE ? S.rc : CJS_E_HIP; break; }
      J.out_off[g0] = 0;                                            // (offsets inside the batch's scratch)
      for (size_t k = g0; k < g1; k++) J.out_off[k + 1] = J.out_off[k] + J.chain[k].out_len;
      uint8_t* d_exp = nullptr;
      if ((rc = S.take((void**)&d_exp, (size_t)J.out_off[g1] + 64)) != 0) break;
      J.dev_out = d_exp; J.host = nullptr;
      guarded(S.rc, [&] { dec_phase_c(&J, &S); });
      if (S.rc) { rc = S.rc; break; }
      // the verdicts, and the good blocks' pieces as runs of the scratch (neighbours in both the scratch and the layout merged)
      struct Run { uint64_t src, to, len; };                        // len bytes from byte src of d_exp to byte `to` of the layout
      std::vector<Run> runs;
      uint64_t packed = 0;
      for (size_t k = g0; k < g1; k++) {
        const uint32_t b = chain_blk[k];
        while (piece_at < P.pieces.size() && P.pieces[piece_at].block < b) piece_at++;
        if (J.chain[k].out_len != ix->e[b].size) continue;
        if (J.crc_got[k] != J.chain[k].crc) { verdict[b] = RG_BAD_CRC; crc_got[b] = J.crc_got[k]; continue; }
        verdict[b] = RG_GOOD;
        for (; piece_at < P.pieces.size() && P.pieces[piece_at].block == b; piece_at++) {
          const RangePiece& p = P.pieces[piece_at];
          const uint64_t src = J.out_off[k] + p.in_off;
          if (!runs.empty() && runs.back().src + runs.back().len == src && runs.back().to + runs.back().len == p.out) runs.back().len += p.len;
          else runs.push_back(Run{src, p.out, p.len});
          packed += p.len;
        }
      }
      // Host form, a few long runs (one long range, the whole stream): each goes from the scratch straight to its place, no
      // gather.  Else the slice gather: into d_out, or into a packed buffer that goes to the host in one copy.
      const bool direct = host_out && runs.size() <= 16;
      std::vector<Slice> sl;
      uint8_t* d_pack = nullptr; Slice* d_sl = nullptr;
      HostGive bounce{nullptr};
      if (!direct && packed) {
        if (host_out && (rc = S.take((void**)&d_pack, (size_t)packed + 64)) != 0) break;
        if (host_out && !(bounce.p = HostPool::take((size_t)packed))) { rc = CJS_E_OUT_OF_MEMORY; break; }
        uint64_t at = 0;
        for (const Run& r : runs) {
          range_slices(sl, (uint64_t)(uintptr_t)(d_exp + r.src), (uint64_t)(uintptr_t)(host_out ? d_pack + at : d_out + r.to), r.len);
          at += r.len;
        }
        if ((rc = S.take((void**)&d_sl, sizeof(Slice) * sl.size())) != 0) break;
        // from here on no way out without the synchronize below: the copy may still be reading `sl`
        if (hipMemcpyAsync(d_sl, sl.data(), sizeof(Slice) * sl.size(), hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
        else {
          S.h2d += sizeof(Slice) * sl.size(); st.slices += sl.size();
          launch_slices(s, d_sl, sl.size());
          if (hipGetLastError() != hipSuccess) rc = CJS_E_HIP;
        }
      }
      if (!rc && host_out && packed) {
        if (direct) { for (const Run& r : runs) if (hipMemcpyAsync(host_out + r.to, d_exp + r.src, (size_t)r.len, hipMemcpyDeviceToHost, s) != hipSuccess) { rc = CJS_E_HIP; break; } }
        else if (hipMemcpyAsync(bounce.p, d_pack, (size_t)packed, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
        S.d2h += packed;
      }
      if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = CJS_E_HIP;
      if (rc) break;
      if (bounce.p) { uint64_t at = 0; for (const Run& r : runs) { memcpy(host_out + r.to, (const uint8_t*)bounce.p + at, (size_t)r.len); at += r.len; } }
      S.drop(d_exp); S.drop(S.d_w); S.drop(S.d_carry);              // (the stream has drained)
      if (d_pack) S.drop(d_pack);
      if (d_sl) S.drop(d_sl);
      S.d_w = nullptr; S.d_carry = nullptr;
      g0 = g1;
    }
    if (rc) return rc;
    if (rows) S.drop(rows);
    st.h2d += S.h2d; st.d2h += S.d2h; st.a_batches += S.a_batches; st.b_batches += S.b_batches;
    S.release_keep_stream(keep);
    t0 = t1;
  }
  return 0;
}

// The verdict of every range from the verdicts of the blocks: status, and the detail of the lowest-index failing range's first bad
// block.  `fail` gets 1 for a failing range.
void range_verdicts(const cjs_bz_index* ix, const RangePlan& P, const uint64_t* off, size_t count, const std::vector<uint8_t>& verdict,
                    const std::vector<uint32_t>& crc_got, int32_t* status, std::vector<uint8_t>& fail) {
  const size_t nblk = ix->e.size();
  std::vector<size_t> next_bad(nblk + 1, nblk);                    // the first bad block at or behind b
  for (size_t b = nblk; b-- > 0;) next_bad[b] = verdict[b] != RG_GOOD ? b : next_bad[b + 1];
  fail.assign(count, 0);
  bool first = true;
  for (size_t k = 0; k < count; k++) {
    status[k] = 0;
    if (!P.lay_len[k]) continue;
    const size_t b0 = P.first_block(ix, off[k]), b1 = P.first_block(ix, off[k] + P.lay_len[k] - 1), bad = next_bad[b0];
    if (bad > b1) continue;
    status[k] = CJS_E_DATA_ERROR; fail[k] = 1;
    if (first) {
      char d[96];
      if (verdict[bad] == RG_BAD_CRC) { bad_crc_detail(d, sizeof d, crc_got[bad], ix->e[bad].crc); set_detail("%s", d); }
      else set_detail("index does not match the stream at block %zu", bad);
      first = false;
    }
  }
}

int range_check_args(const void* in, size_t n, const cjs_bz_index* idx, const uint64_t* off, const uint64_t* len, size_t count, const size_t* out_off,
                     const size_t* out_len, const int32_t* status) {
  if (!idx || (!in && n)) return CJS_E_INVALID_ARG;
  if (count && (!off || !len || !out_off || !out_len || !status)) return CJS_E_INVALID_ARG;
  if (idx->stream_bytes != n) { set_detail("the index is of a stream of %llu bytes", (unsigned long long)idx->stream_bytes); return CJS_E_INVALID_ARG; }
  return 0;
}

void range_debug(const char* form, const cjs_bz_index* ix, const RangePlan& P, size_t count, const RangeStats& st) {
  if (!env_debug()) return;
  fprintf(stderr, "[cjs range] %s: %zu ranges, %llu bytes, %zu of %zu blocks touched, %u passes (%u row batches, %u inverse-BWT batches), upload %llu B, %zu slices, H2D %llu D2H %llu\n",
          form, count, (unsigned long long)P.total, P.touched.size(), ix->e.size(), st.passes, st.a_batches, st.b_batches, (unsigned long long)st.up, st.slices,
          (unsigned long long)st.h2d, (unsigned long long)st.d2h);
}

}  // namespace

extern "C" int cjs_bzip2_index_build(const uint8_t* in, size_t n, int multistream, cjs_bz_index** idx, const cjs_opts* opts) {
  if (!idx) return CJS_E_INVALID_ARG;
  *idx = nullptr;
  CJS_GUARD_BEGIN
  long nbk = 0;
  std::vector<cjs_bz_index_entry> e;
  CJS_TRY(bunzip_core(in, n, multistream, 1, 0, nullptr, nullptr, nullptr, nullptr, 0, &nbk, opts, &e));
  e.resize((size_t)nbk);
  return bz_index_make(e.data(), e.size(), n, multistream != 0, idx);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_read_ranges(const uint8_t* in, size_t n, const cjs_bz_index* idx, const uint64_t* off, const uint64_t* len, size_t count,
                                     uint8_t** out, size_t* out_off, size_t* out_len, int32_t* status, const cjs_opts* opts) {
  if (!out) return CJS_E_INVALID_ARG;
  *out = nullptr;
  clear_detail();
  CJS_GUARD_BEGIN
  CJS_TRY(range_check_args(in, n, idx, off, len, count, out_off, out_len, status));
  RangePlan P;
  CJS_TRY(range_plan(idx, off, len, count, P));
  RecHost host;                                                   // (given back on every failing path)
  CJS_TRY(host.ensure(0, (size_t)std::max<uint64_t>(P.total, 1)));
  std::vector<uint8_t> verdict(idx->e.size(), RG_GOOD), fail; std::vector<uint32_t> crc_got(idx->e.size(), 0);
  RangeStats st;
  if (!P.touched.empty()) {
    CJS_TRY(select_device(opts));
    int ndev = 0, dev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CJS_E_NO_DEVICE;
    RestoreDevice restore{dev};
    CJS_TRY(range_run(in, nullptr, idx, P, host.p, nullptr, verdict, crc_got, dev, st));
  }
  range_verdicts(idx, P, off, count, verdict, crc_got, status, fail);
  size_t at = 0;                                                   // the layout behind the verdicts: a failed range takes no room
  for (size_t k = 0; k < count; k++) {
    out_off[k] = at; out_len[k] = fail[k] ? 0 : (size_t)P.lay_len[k];
    if (out_len[k] && at != P.lay_off[k]) memmove(host.p + at, host.p + P.lay_off[k], out_len[k]);
    at += out_len[k];
  }
  range_debug("host", idx, P, count, st);
  *out = host.release();
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_read_ranges_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const uint64_t* off, const uint64_t* len, size_t count,
                                            uint8_t* d_out, size_t out_cap, size_t* out_off, size_t* out_len, int32_t* status, size_t* out_need,
                                            const cjs_opts* opts) {
  if (!out_need || (!d_out && out_cap)) return CJS_E_INVALID_ARG;
  *out_need = 0;
  clear_detail();
  CJS_GUARD_BEGIN
  CJS_TRY(range_check_args(d_in, n, idx, off, len, count, out_off, out_len, status));
  RangePlan P;
  CJS_TRY(range_plan(idx, off, len, count, P));
  *out_need = (size_t)P.total;
  for (size_t k = 0; k < count; k++) { out_off[k] = (size_t)P.lay_off[k]; out_len[k] = (size_t)P.lay_len[k]; status[k] = 0; }
  if (P.total > out_cap) return CJS_E_OUTPUT_TOO_SMALL;           // (known from the index alone: nothing is launched, d_out untouched)
  if (P.touched.empty()) return 0;
  CJS_TRY(select_device(opts));
  int ndev = 0, dev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CJS_E_NO_DEVICE;
  RestoreDevice restore{dev};
  if (!on_device(d_in, dev) || !on_device(d_out, dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  std::vector<uint8_t> verdict(idx->e.size(), RG_GOOD), fail; std::vector<uint32_t> crc_got(idx->e.size(), 0);
  RangeStats st;
  CJS_TRY(range_run(nullptr, d_in, idx, P, nullptr, d_out, verdict, crc_got, dev, st));
  range_verdicts(idx, P, off, count, verdict, crc_got, status, fail);
  for (size_t k = 0; k < count; k++) if (fail[k]) out_len[k] = 0;      // (the region keeps its place)
  range_debug("device", idx, P, count, st);
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// ---------------------------------------------------------------- batch (Bzip2.decompressFiles)
// The groups above with the inputs and the result in host memory: a group's inputs are staged into one host buffer and uploaded
// as phase A uploads a single stream; phase C copies the bytes back into a result buffer of the group.  See DESIGN.md §6c.
namespace {

struct BatchPiece { uint8_t* buf; size_t size; };       // a HostPool result buffer and the bytes used in it

// one group: inputs [k0, k1); every status / off (inside the group's piece) / len and detail is set
int dec_batch_group(const uint8_t* const* in, const size_t* n, size_t k0, size_t k1, int multistream, int dev, size_t* off, size_t* len,
                    int32_t* status, std::vector<std::string>& detail, BatchPiece* piece) {
  piece->buf = nullptr; piece->size = 0;
  DecJob J; DecShare S; BatchGroup G;
  S.device = dev;
  for (size_t k = k0; k < k1; k++) off[k] = len[k] = 0;
  group_layout(J, S, G, k0, k1, n, status, detail, [&](size_t k) { return in[k]; },
               [&](size_t k, int level) { return bz_max_level(in[k], n[k], level, multistream != 0); }, [](size_t, size_t) {});
  uint8_t* host_in = (uint8_t*)HostPool::take(J.n ? J.n : 1);
  if (!host_in) return CJS_E_OUT_OF_MEMORY;
  struct GiveBack { uint8_t* p; ~GiveBack() { HostPool::give(p); } } give_in{host_in};
  for (size_t k = k0; k < k1; k++) if (G.ok[k - k0]) memcpy(host_in + S.bst[k - k0], in[k], n[k]);
  J.in = host_in;
  uint64_t total = 0;
  CJS_TRY(group_prepare(J, S, G, status, detail, [&](size_t k, const WalkCands& C) { return walk_chain(J, C, in[k], n[k], multistream, 0, met_nothing); }, &total));
  const size_t nb = J.chain.size();
  J.host = (uint8_t*)HostPool::take(total ? (size_t)total : 1);
  if (!J.host) return CJS_E_OUT_OF_MEMORY;
  J.crc_got.assign(nb, 0);
  if (nb) guarded(S.rc, [&] { dec_phase_c(&J, &S); });
  S.release();                                                 // (the stream has drained before J.host is read or given back)
  if (S.rc) { HostPool::give(J.host); return S.rc; }
  group_verdicts(J, G, 0, off, len, status, detail);
  if (J.timing)
    fprintf(stderr, "[cjs dec batch] group: %zu inputs, %zu candidates, %u row batches (phase A), %u inverse-BWT batches (phase B), %zu chain blocks, %llu bytes out\n",
            k1 - k0, S.cands.size(), S.a_batches, S.b_batches, nb, (unsigned long long)total);
  piece->buf = J.host; piece->size = (size_t)total;
  return 0;
}

}  // namespace

extern "C" int cjs_bzip2_decompress_batch(const uint8_t* const* in, const size_t* n, size_t count, int multistream, uint8_t** out, size_t* off,
                                          size_t* len, int32_t* status, const cjs_opts* opts) {
  if (!out) return CJS_E_INVALID_ARG;
  *out = nullptr;
  clear_detail();
  if (count == 0) return 0;
  if (!in || !n || !off || !len || !status) return CJS_E_INVALID_ARG;
  for (size_t k = 0; k < count; k++) if (n[k] && !in[k]) return CJS_E_INVALID_ARG;
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  int dev = 0, ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CJS_E_NO_DEVICE;
  RestoreDevice restore{dev};
  cjs_opts one; memset(&one, 0, sizeof one);                   // (the large inputs: this device, n_devices and stats ignored)
  one.struct_size = sizeof one; one.device = dev;
  const size_t G = dec_group_bytes();
  std::vector<std::string> detail(count);
  std::vector<BatchPiece> pieces;
  std::vector<size_t> piece_of(count);
  struct Pieces { std::vector<BatchPiece>& v; ~Pieces() { for (auto& p : v) HostPool::give(p.buf); } } keep{pieces};
  int rc = 0;
  for (size_t k0 = 0; k0 < count && !rc;) {
    if (n[k0] > G) {                                           // an input of its own: the single-stream path
      uint8_t* o = nullptr; size_t on = 0;
      const int r = cjs_bzip2_decompress(in[k0], n[k0], multistream, &o, &on, &one);
      if (r == CJS_E_OUT_OF_MEMORY || r == CJS_E_NO_DEVICE || r == CJS_E_HIP || r == CJS_E_INVALID_ARG) { rc = r; break; }
      status[k0] = r; off[k0] = 0; len[k0] = r ? 0 : on;
      if (r) detail[k0] = cjs_last_error_detail();
      else { pieces.push_back(BatchPiece{o, on}); piece_of[k0] = pieces.size() - 1; }
      if (r) { piece_of[k0] = pieces.size(); pieces.push_back(BatchPiece{nullptr, 0}); }
      k0++;
      continue;
    }
    const size_t k1 = dec_group_end(n, count, k0, G);
    BatchPiece p{nullptr, 0};
    if ((rc = dec_batch_group(in, n, k0, k1, multistream, dev, off, len, status, detail, &p)) != 0) break;
    pieces.push_back(p);
    for (size_t k = k0; k < k1; k++) piece_of[k] = pieces.size() - 1;
    k0 = k1;
  }
  clear_detail();
  if (rc) return rc;
  uint8_t* res = nullptr;
  if (pieces.size() == 1 && pieces[0].buf) { res = pieces[0].buf; pieces[0].buf = nullptr; }      // (one group: its buffer is the result)
  else {
    std::vector<size_t> base(pieces.size() + 1, 0);
    for (size_t i = 0; i < pieces.size(); i++) base[i + 1] = base[i] + pieces[i].size;
    if (!(res = (uint8_t*)HostPool::take(base.back() ? base.back() : 1))) return CJS_E_OUT_OF_MEMORY;
    for (size_t i = 0; i < pieces.size(); i++) if (pieces[i].size) memcpy(res + base[i], pieces[i].buf, pieces[i].size);
    for (size_t k = 0; k < count; k++) off[k] += base[piece_of[k]];
  }
  *out = res;
  for (size_t k = 0; k < count; k++) if (status[k]) { set_detail("%s", detail[k].c_str()); break; }      // the lowest-index failing input's
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// ---------------------------------------------------------------- device-resident batch (cjs_bzip2_decompress_batch_device)
// cjs_bzip2_decompress_batch with the inputs and the result in GPU memory: the same groups (dec_group_bytes), verdicts and layout.
// Every group and every input above the group size (the single device path) is prepared up to phase B first -- the single
// ones also through a CRC-only phase C, as a failed one takes no bytes -- so the layout and its size are known before anything
// is written; then each emits into its region of d_out.  See DESIGN.md §6d.
extern "C" int cjs_bzip2_decompress_batch_device(const uint8_t* d_in, const size_t* in_off, size_t count, int multistream, uint8_t* d_out, size_t out_cap,
                                                 size_t* out_off, size_t* out_len, int32_t* status, size_t* out_need, const cjs_opts* opts) {
  clear_detail();
  if (count == 0) { if (out_need) *out_need = 0; return 0; }
  if (!in_off || !out_off || !out_len || !status || !out_need || count >= 0xFFFFFFFFu) return CJS_E_INVALID_ARG;
  for (size_t k = 0; k < count; k++) if (in_off[k + 1] < in_off[k]) return CJS_E_INVALID_ARG;
  if ((!d_in && in_off[count] > in_off[0]) || (!d_out && out_cap)) return CJS_E_INVALID_ARG;
  *out_need = 0;
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  int ndev = 0, dev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CJS_E_NO_DEVICE;
  RestoreDevice restore{dev};
  if ((in_off[count] > in_off[0] && !on_device(d_in + in_off[0], dev)) || (out_cap && !on_device(d_out, dev))) return CJS_E_INVALID_ARG;
  DecShare H;                                                   // the header pass: its stream, pool and copy tally
  H.device = dev;
  std::vector<DevHdr> hd;
  CJS_TRY(dev_headers(H, d_in, std::vector<uint64_t>(in_off, in_off + count + 1), multistream != 0, hd));
  H.release();
  const size_t G = dec_group_bytes();
  std::vector<size_t> n(count);
  for (size_t k = 0; k < count; k++) n[k] = in_off[k + 1] - in_off[k];
  std::vector<std::string> detail(count);
  std::vector<std::unique_ptr<DevUnit>> units;
  std::vector<size_t> unit_base;
  uint64_t need = 0;
  for (size_t k0 = 0; k0 < count;) {
    units.emplace_back(new DevUnit);
    DevUnit& U = *units.back();
    U.S.device = dev;
    if (n[k0] > G) {                                            // an input of its own: the single device path
      U.G.k0 = k0; U.G.k1 = k0 + 1;
      clear_detail();
      int r = dev_single_prepare(U, d_in + in_off[k0], n[k0], multistream, hd[k0]);
      if (!r) r = dev_single_emit(U, nullptr);                  // (the verdict: a failed input takes no bytes)
      if (r == CJS_E_OUT_OF_MEMORY || r == CJS_E_NO_DEVICE || r == CJS_E_HIP || r == CJS_E_INVALID_ARG) return r;
      status[k0] = r;
      if (r) { detail[k0] = cjs_last_error_detail(); U.S.release(); }
      unit_base.push_back((size_t)need);
      out_off[k0] = (size_t)need; out_len[k0] = r ? 0 : (size_t)U.total;
      need += r ? 0 : U.total;
      k0++;
      continue;
    }
    const size_t k1 = dec_group_end(n.data(), count, k0, G);
    CJS_TRY(dev_group_prepare(U, d_in, in_off, n.data(), k0, k1, multistream, hd, status, detail));
    unit_base.push_back((size_t)need);
    need += U.total;
    k0 = k1;
  }
  clear_detail();
  *out_need = (size_t)need;
  uint64_t h2d = H.h2d, d2h = H.d2h, cands = 0, blocks = 0;
  auto tally = [&]() {
    for (auto& u : units) { h2d += u->S.h2d; d2h += u->S.d2h; cands += u->S.cands.size(); blocks += u->J.chain.size(); }
    if (env_debug())
      fprintf(stderr, "[cjs dec dev] batch: %zu inputs, %zu units, %llu bytes out, H2D %llu D2H %llu candidates %llu blocks %llu\n", count, units.size(),
              (unsigned long long)need, (unsigned long long)h2d, (unsigned long long)d2h, (unsigned long long)cands, (unsigned long long)blocks);
  };
  if (need > out_cap) { tally(); return CJS_E_OUTPUT_TOO_SMALL; }      // (d_out untouched)
  for (size_t u = 0; u < units.size(); u++) {
    DevUnit& U = *units[u];
    if (U.J.batch) CJS_TRY(dev_group_emit(U, d_out + unit_base[u], unit_base[u], out_off, out_len, status, detail));
    else if (!status[U.G.k0] && dev_single_emit(U, d_out + unit_base[u]) != 0) return CJS_E_HIP;      // (its verdict was 0 a moment ago)
    U.S.release();
  }
  tally();
  clear_detail();
  for (size_t k = 0; k < count; k++) if (status[k]) { set_detail("%s", detail[k].c_str()); break; }      // the lowest-index failing input's
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

// ---------------------------------------------------------------- streaming decode (cjs_bzip2_dec_*)
// The phases above over a sliding window of the stream.  The decoder keeps the stream bytes from the carry point on (host copy;
// uploaded per step at their absolute byte offset, so the dword phase holds), the walk state (WalkState: bit position, folded
// stream CRC, the member's block size) and one output buffer of out_bytes.  A step: phase A over the window with rows for the
// first R block candidates at the walk position; bz_walk resumed from the kept state, stopping in front of whatever the bytes
// still to come could change; phase B over the chain; the chain cut to the output budget (the walk state rolled back to the first
// block not emitted); phase C into the device output buffer and one D2H.  All device scratch comes from the decoder's DecArena.
// Synchronous: no worker thread.  See DESIGN.md §6f.
namespace {
constexpr size_t DEC_DEFAULT_CHUNK = (size_t)64 << 20, DEC_DEFAULT_OUT = (size_t)256 << 20;      // DESIGN.md §6f (placeholders, UNMEASURED)
constexpr size_t DEC_MIN_CHUNK = (size_t)64 << 10, DEC_MAX_CHUNK = (size_t)1 << 30;
const char* const WALK_WHY[] = {"runs", "end of stream", "block magic not all here", "stream crc not all here", "member header not all here", "candidate without a row",
                                "block not all here", "error too near the end", "output budget"};
struct WinBytes {                        // the window by absolute stream byte
  const uint8_t* p; uint64_t off;
  uint8_t operator[](uint64_t i) const { return p[i - off]; }
};
}  // namespace

struct cjs_bz_dec {
  int multistream = 0, device = -1;
  size_t chunk = 0, out_req = 0;
  bool eager = false, debug = false;
  int rc = 0; char detail[192] = {0};      // first failure: every later call returns it
  // input window: stream bytes [win_off, win_off + win_len); the first `seen` of them have been through a step
  uint8_t* win = nullptr; size_t win_cap = 0, win_len = 0, seen = 0; uint64_t win_off = 0, written = 0;
  bool win_pinned = false, finished = false, header_ok = false, ended = false, dev_ready = false;
  int level = 0;                           // of the header; rows and blocks are sized for L = 9 with multistream
  uint32_t tt_stride = 0, rows = 0;
  WalkState W;
  // output of the last step: held - held_pos bytes still to be read; then the pending verdict
  size_t out_cap = 0, held = 0, held_pos = 0;
  Pinned<uint8_t> h_out; DevMem<uint8_t> d_out;
  int pend_rc = 0; char pend_detail[192] = {0};
  DecArena arena; Stream s;
  uint32_t steps = 0;
  int fail(int code, const char* text) {
    if (!rc) { rc = code; snprintf(detail, sizeof detail, "%s", text ? text : ""); }
    clear_detail();
    if (detail[0]) set_detail("%s", detail);
    return rc;
  }
  ~cjs_bz_dec() {
    int cur = 0;
    if (dev_ready && hipGetDevice(&cur) == hipSuccess) {
      RestoreDevice restore{cur};          // the caller's device stays current
      if (hipSetDevice(device) == hipSuccess) {
        if (s) (void)hipStreamSynchronize(s);
        if (win_pinned) (void)hipHostUnregister(win);
        s.reset(); h_out.reset(); d_out.reset(); arena.release();
      }
    }
    free(win);
  }
};

namespace {

// _start_bunzip (:1408-1427) on the first four bytes: no device
int dec_header(cjs_bz_dec* d) {
  const char* why = nullptr;
  if (bz_header_check(d->win, d->written, &d->level, &why)) return d->fail(CJS_E_NOT_BZIP_DATA, why);
  const uint32_t L = d->multistream ? 9u : (uint32_t)d->level;      // later members cannot be seen ahead
  d->tt_stride = 100000u * L;
  d->out_cap = std::max<size_t>(d->out_req ? d->out_req : DEC_DEFAULT_OUT, (size_t)52 * d->tt_stride);
  d->rows = (uint32_t)std::min<size_t>(65535, std::max<size_t>(1, d->out_cap / d->tt_stride));
  d->W = WalkState{};
  d->W.dbuf_size = 100000u * (uint32_t)d->level;
  d->header_ok = true;
  return 0;
}

int dec_device_init(cjs_bz_dec* d) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return CJS_E_NO_DEVICE; }
  if (d->device >= ndev) return CJS_E_INVALID_ARG;
  if (d->device < 0 && hipGetDevice(&d->device) != hipSuccess) return CJS_E_NO_DEVICE;
  CJS_HIP_TRY(hipSetDevice(d->device));
  d->dev_ready = true;
  CJS_HIP_TRY(hipStreamCreate(d->s.put()));
  if (hipHostRegister(d->win, d->win_cap, hipHostRegisterDefault) == hipSuccess) d->win_pinned = true; else (void)hipGetLastError();
  CJS_HIP_TRY(hipHostMalloc((void**)d->h_out.put(), d->out_cap));
  CJS_TRY(d->d_out.alloc(d->out_cap + 256));
  // rows ~10 B and inverse BWT ~24 B per byte of rows x block size, the window twice (upload + candidates)
  return d->arena.init((size_t)28 * d->rows * ((size_t)d->tt_stride + 4096) + 2 * d->win_cap + ((size_t)16 << 20));
}

int dec_step(cjs_bz_dec* d) {
  int cur = 0;
  if (!d->dev_ready) {
    const bool had = hipGetDevice(&cur) == hipSuccess;
    const int rc = dec_device_init(d);
    if (rc) { if (had) (void)hipSetDevice(cur); return rc; }
    if (had) (void)hipSetDevice(cur);
  }
  if (hipGetDevice(&cur) != hipSuccess) return CJS_E_NO_DEVICE;
  RestoreDevice restore{cur};
  CJS_HIP_TRY(hipSetDevice(d->device));
  const bool final = d->finished, was_full = d->win_len == d->win_cap;
  const uint32_t spills0 = d->arena.spills;
  const uint64_t n = d->win_off + d->win_len, pos0 = d->W.pos;
  const size_t len0 = d->win_len;
  DecJob J; J.n = (size_t)n; J.mode = 0; J.timing = env_debug(); J.tt_stride = d->tt_stride; J.batch = true;
  DecShare S; S.device = d->device; S.arena = &d->arena; S.s = std::move(d->s);
  struct Back { cjs_bz_dec* d; DecShare& S; ~Back() { S.release_keep_stream(d->s); } } back{d, S};      // on every path out
  S.lo = S.up_lo = d->win_off; S.hi = S.up_hi = n; S.row_limit = d->rows; S.row_from = d->W.pos;
  J.upload = [d](DecShare* sh, uint8_t* dst) {
    if (d->win_len && hipMemcpyAsync(dst, d->win, d->win_len, hipMemcpyHostToDevice, sh->s) != hipSuccess) return (int)CJS_E_HIP;
    sh->h2d += d->win_len;
    return 0;
  };
  guarded(S.rc, [&] { dec_phase_a(&J, &S); });
  if (S.rc) return S.rc;
  // ---- the walk, resumed
  WalkState& W = d->W;
  W.partial = !final; W.cut_bit = S.cut_bit; W.extent = dec_extent(d->tt_stride); W.stop = WALK_RUNS;
  std::vector<WalkState> before;           // the state in front of each chain block
  clear_detail();
  int wrc = walk_chain(J, WalkCands(&S, 1), WinBytes{d->win, d->win_off}, (size_t)n, d->multistream, 0,
                       [&](long ci, uint64_t) { if (S.cands[(size_t)ci].kind == 0) before.push_back(W); }, &W);
  char wdetail[192];
  snprintf(wdetail, sizeof wdetail, "%s", cjs_last_error_detail());
  clear_detail();
  // ---- phase B over the chain, then the cut to the output budget
  size_t nb = J.chain.size();
  const size_t walked = nb;
  if (nb) {
    S.c0 = 0; S.c1 = nb;
    guarded(S.rc, [&] { dec_phase_b(&J, &S); });
    if (S.rc) return S.rc;
  }
  chain_out_offsets(J);
  if (nb) {
    if (J.out_off[1] > d->out_cap) return CJS_E_UNSUPPORTED;      // cannot happen: out_cap >= a block's largest expansion
    size_t k = 1;
    while (k < nb && J.out_off[k + 1] <= d->out_cap) k++;
    if (k < nb) {                          // block k and what the walk met behind it: the next step's
      const WalkState& b = before[k];
      W.pos = b.pos; W.crc = b.crc; W.dbuf_size = b.dbuf_size; W.stop = WALK_OUT_BUDGET;
      wrc = 0;
      J.chain.resize(k); J.out_off.resize(k + 1); S.c1 = nb = k;
    }
    // ---- phase C: a CRC verdict per block; the first bad block in chain order comes before the walk's error
    J.dev_out = d->d_out; J.host = nullptr; J.crc_got.assign(nb, 0);
    S.rc = 0;
    guarded(S.rc, [&] { dec_phase_c(&J, &S); });
    if (S.rc) return S.rc;
  }
  size_t bad = 0;
  while (bad < nb && J.crc_got[bad] == J.chain[bad].crc) bad++;
  const size_t deliver = (size_t)J.out_off[bad];
  if (deliver) { CJS_HIP_TRY(hipMemcpyAsync(d->h_out, d->d_out, deliver, hipMemcpyDeviceToHost, S.s)); CJS_HIP_TRY(hipStreamSynchronize(S.s)); S.d2h += deliver; }
  d->held = deliver; d->held_pos = 0;
  if (bad < nb) {                          // Bad block CRC (:1756-1761): nothing of the block is delivered
    d->pend_rc = CJS_E_DATA_ERROR;
    bad_crc_detail(d->pend_detail, sizeof d->pend_detail, J.crc_got[bad], J.chain[bad].crc);
  } else if (wrc) {
    d->pend_rc = wrc;
    snprintf(d->pend_detail, sizeof d->pend_detail, "%s", wdetail);
  } else if (W.stop == WALK_ENDED) d->ended = true;
  // ---- the carry: the window from the walk position's byte on
  if (!d->pend_rc) {
    const uint64_t keep_from = d->ended ? n : std::min<uint64_t>(W.pos >> 3, n);
    const size_t gone = (size_t)(keep_from - d->win_off);
    if (gone) memmove(d->win, d->win + gone, d->win_len - gone);
    d->win_off = keep_from; d->win_len -= gone;
  }
  d->seen = d->win_len;
  if (d->debug)
    fprintf(stderr, "[cjs dec step] %u: window %zu B at byte %llu, carry %zu B, candidates %u rows %u, blocks walked %zu emitted %zu, %zu B out, walk stopped: %s%s%s\n",
            d->steps, len0, (unsigned long long)(n - len0), d->win_len, S.ncand_seen, S.nrows_given(), walked, std::min(bad, nb), deliver,
            d->pend_rc ? "error" : WALK_WHY[W.stop], final ? " (final)" : "", d->arena.spills != spills0 ? " [arena spilled]" : "");
  d->steps++;
  // (cannot happen: a full window holds a whole block behind the walk position, and the final steps end or emit)
  if (!d->pend_rc && !d->ended && (final ? W.pos == pos0 : was_full && d->win_len == d->win_cap)) return CJS_E_UNSUPPORTED;
  return 0;
}

// A full window always has fresh bytes: the step that last ran on a full window either moved the walk position, and with it the
// carry point (a block, an end-of-stream record or a member header: whole bytes each), so the window was no longer full and only
// a _write can have filled it again; or it failed the decoder (CJS_E_UNSUPPORTED in dec_step).  So a _write that took nothing is
// always followed by a step.
bool dec_step_due(const cjs_bz_dec* d) {
  if (d->ended || d->pend_rc) return false;
  if (d->finished) return true;
  const size_t fresh = d->win_len - d->seen;
  return d->eager ? fresh > 0 : (fresh >= d->chunk || (d->win_len == d->win_cap && fresh > 0));
}

}  // namespace

extern "C" int cjs_bzip2_dec_create(cjs_bz_dec** out, int multistream, size_t chunk_bytes, size_t out_bytes, const cjs_opts* opts) {
  if (!out) return CJS_E_INVALID_ARG;
  *out = nullptr;
  CJS_GUARD_BEGIN
  cjs_bz_dec* d = new cjs_bz_dec();
  d->multistream = multistream ? 1 : 0;
  if (!chunk_bytes) {                      // the default; CJS_DEC_CHUNK_BYTES replaces it (callers without a chunk argument: the JS fronts, cli.js)
    const char* env = getenv("CJS_DEC_CHUNK_BYTES");
    chunk_bytes = env ? (size_t)strtoull(env, nullptr, 10) : 0;
    if (!chunk_bytes) chunk_bytes = DEC_DEFAULT_CHUNK;
  }
  d->chunk = std::min(std::max(chunk_bytes, DEC_MIN_CHUNK), DEC_MAX_CHUNK);
  d->out_req = out_bytes;
  d->device = Opts(opts).device;
  const char* eager = getenv("CJS_DEC_STREAM_EAGER");
  d->eager = eager && eager[0] == '1';
  d->debug = getenv("CJS_DEBUG") != nullptr;
  d->win_cap = d->chunk + (size_t)dec_extent(900000u);
  *out = d;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_dec_write(cjs_bz_dec* d, const uint8_t* in, size_t n, size_t* taken) {
  if (taken) *taken = 0;
  if (!d) return CJS_E_INVALID_ARG;
  if (d->rc) return d->fail(d->rc, nullptr);
  if (!taken || (!in && n) || d->finished) return d->fail(CJS_E_INVALID_ARG, nullptr);
  if (d->ended || d->pend_rc) { *taken = n; return 0; }      // the end has been decided: the reference never reads these bytes
  if (!n) return 0;
  if (!d->win && !(d->win = (uint8_t*)malloc(d->win_cap))) return d->fail(CJS_E_OUT_OF_MEMORY, nullptr);
  const size_t take = std::min(n, d->win_cap - d->win_len);
  memcpy(d->win + d->win_len, in, take);
  d->win_len += take; d->written += take;
  *taken = take;
  return 0;
}

extern "C" int cjs_bzip2_dec_finish(cjs_bz_dec* d) {
  if (!d) return CJS_E_INVALID_ARG;
  if (d->rc) return d->fail(d->rc, nullptr);
  d->finished = true;
  return 0;
}

extern "C" int cjs_bzip2_dec_read(cjs_bz_dec* d, uint8_t* out, size_t cap, size_t* got) {
  if (got) *got = 0;
  if (!d) return CJS_E_INVALID_ARG;
  if (d->rc) return d->fail(d->rc, nullptr);
  if (!got || (!out && cap)) return d->fail(CJS_E_INVALID_ARG, nullptr);
  CJS_GUARD_BEGIN
  for (;;) {
    if (d->held_pos < d->held) {
      const size_t take = std::min(cap, d->held - d->held_pos);
      if (take) memcpy(out, d->h_out.p + d->held_pos, take);
      d->held_pos += take;
      *got = take;
      return 0;
    }
    if (d->pend_rc) return d->fail(d->pend_rc, d->pend_detail);      // every byte in front of it has been read
    if (d->ended) return 0;
    if (!d->header_ok) {
      if (d->written < 4 && !d->finished) return 0;
      CJS_TRY(dec_header(d));
    }
    if (!dec_step_due(d)) return 0;
    if (!d->win && !(d->win = (uint8_t*)malloc(d->win_cap))) return d->fail(CJS_E_OUT_OF_MEMORY, nullptr);
    const int rc = dec_step(d);
    if (rc) return d->fail(rc, cjs_last_error_detail());
  }
  CJS_GUARD_END(d->fail(CJS_E_OUT_OF_MEMORY, nullptr), d->fail(CJS_E_HIP, nullptr))
}

extern "C" int cjs_bzip2_dec_done(const cjs_bz_dec* d) { return d && !d->rc && d->ended && d->held_pos == d->held ? 1 : 0; }

extern "C" void cjs_bzip2_dec_destroy(cjs_bz_dec* d) { delete d; }
