// decode.hip — Bzip2.decompressFile (Bunzip.decode, J/Bzip2_joined_.js:1769-1796) on the MI355X: the decode kernels, the engine
// that runs them in three phases (dec_engine.h) and the single-stream driver.  The other drivers of the engine have files of
// their own: dec_batch.hip (host batch, device-resident single and batch), dec_recover.hip, range.hip, dec_stream.hip.
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
// Recovery of damaged data (dec_recover.hip: cjs_bzip2_recover, no reference equivalent: the job of bzip2recover) is 1, 2 and 4-6
// over EVERY decodable candidate, with step 3 replaced by a selection of the intact, non-overlapping ones; an indexed range read
// (range.hip) is 2 and 4-6 over the blocks its index names.
#include "dec_engine.h"
#include "prims.hpp"
#include "rle1.h"
#include <stdlib.h>
#include <string.h>

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

// ---------------------------------------------------------------- 4. inverse BWT (IbBlock, a block of a batch: dec_engine.h)
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
// Eight drivers sit on the phases, through dec_engine.h (the arena, the share, the job, the walk and the glue between the phases):
//   here             bunzip_core (single stream, shares over devices; cjs_bzip2_decompress, _decompress_block, _table, and the
//                    table pass of cjs_bzip2_index_build)
//   dec_batch.hip    dec_batch_group (host batch), dev_single_* (device-resident single stream), dev_group_* (device-resident batch)
//   dec_recover.hip  recover_core (recovery, both forms)
//   range.hip        range_run (indexed range reads, both forms)
//   dec_stream.hip   dec_step (streaming)
// A driver holds what is particular to it: where the bytes come from and where they go.
namespace cjs {

constexpr uint64_t DEC_BATCH_ELEMS = 1ull << 28;      // BWT bytes per inverse-BWT batch (scratch ~ 21 B each)

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

// _start_bunzip (:1408-1427) on the first four bytes h of an input (or of a member stream) of n bytes: 0 and the level, or
// CJS_E_NOT_BZIP_DATA and the detail text in *why (the caller sets it, or stores it with its input)
int bz_header_check(const uint8_t* h, size_t n, int* level, const char** why) {
  if (n < 4 || h[0] != 'B' || h[1] != 'Z' || h[2] != 'h') { *why = "bad magic"; return CJS_E_NOT_BZIP_DATA; }
  *level = h[3] - '0';
  if (*level < 1 || *level > 9) { *why = "level out of range"; return CJS_E_NOT_BZIP_DATA; }
  return 0;
}

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

// exclusive prefix sum of the chain's decoded lengths (phase B's) -> J.out_off; returns the total
uint64_t chain_out_offsets(DecJob& J) {
  const size_t nb = J.chain.size();
  J.out_off.assign(nb + 1, 0);
  for (size_t k = 0; k < nb; k++) J.out_off[k + 1] = J.out_off[k] + J.chain[k].out_len;
  return J.out_off[nb];
}

// ---------------------------------------------------------------- the single-stream driver
int bunzip_core(const uint8_t* in, size_t n, int multistream, int mode, uint64_t at_bit, uint8_t** out, size_t* out_n,
                uint64_t* tab_pos, uint32_t* tab_size, long tab_cap, long* tab_n, const cjs_opts* opts,
                std::vector<cjs_bz_index_entry>* tab_ix) {      // (mode 1: an index entry per block as well)
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
  HostBuf host;                                                                 // (in front of the shares: given back once their streams have drained)
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
  if (out && !pending_rc) { host = HostBuf(total ? (size_t)total : 1); if (!(J.host = host.p)) return CJS_E_OUT_OF_MEMORY; }
  const auto T2 = std::chrono::steady_clock::now();
  rc = for_each_share(sh, &J, dec_phase_c);
  const double ms_c = ms_since(T2);
  for (auto& x : sh) x.release();                              // (the streams have drained before J.host can go back)
  if (J.timing) {
    fprintf(stderr, "[cjs dec] %u share(s): upload + magic scan + block decode %.2f ms, inverse BWT + RLE1 lengths %.2f ms, RLE1 + CRC + D2H %.2f ms\n", nsh, ms_a, ms_b, ms_c);
    for (uint32_t i = 0; i < nsh; i++) fprintf(stderr, "[cjs dec]   share %u (device %d): %zu candidates, blocks [%zu, %zu): %.2f / %.2f / %.2f ms\n", i, sh[i].device,
                                               sh[i].cands.size(), sh[i].c0, sh[i].c1, sh[i].ms_a, sh[i].ms_b, sh[i].ms_c);
  }
  if (rc) return rc;
  if (pending_rc) { set_detail("%s", pending_detail); return pending_rc; }
  if (tab_n) {
    *tab_n = (long)nb;
    for (size_t k = 0; k < nb && (long)k < tab_cap; k++) { tab_pos[k] = J.chain_bits[k]; tab_size[k] = J.chain[k].out_len; }
    if (tab_ix) for (size_t k = 0; k < nb; k++) (*tab_ix)[k].size = J.chain[k].out_len;
  }
  if (out) { *out = host.release(); *out_n = (size_t)total; }
  return 0;
}

}  // namespace cjs

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
