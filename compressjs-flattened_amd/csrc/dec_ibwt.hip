// dec_ibwt.hip — step 4 of the Bzip2 decoder (the map: decode.hip): the inverse-BWT kernels, phase B of the engine (dec_engine.h)
// over the cyclic form, and next to it the same sequence over the sentinel form for BWTC.decompressFile.
#include "dec_engine.h"
#include "prims.hpp"
#include <stdlib.h>

using namespace cjs;

namespace cjs {

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
// ---------------------------------------------------------------- phase B: inverse BWT (T vector by a stable radix pass, splitter list ranking, second walk) + RLE1 length pass
constexpr uint64_t DEC_BATCH_ELEMS = 1ull << 28;      // BWT bytes per inverse-BWT batch (scratch ~ 21 B each)

// batches of the share's chain blocks: [b0, b1) with <= DEC_BATCH_ELEMS elements and <= DEC_BATCH_BLOCKS blocks
size_t dec_next_batch(const DecJob* J, size_t b0, size_t c1) {
  static const uint64_t max_el = getenv("CJS_DEC_BATCH_ELEMS") ? strtoull(getenv("CJS_DEC_BATCH_ELEMS"), nullptr, 10) : DEC_BATCH_ELEMS;   // (tests shrink it)
  return ib_batch_end(b0, c1, max_el, DEC_BATCH_BLOCKS, [&](size_t k) { return J->chain[k].count; });
}

// scratch of one inverse-BWT batch
struct IbScratch {
  IbBlock* d_blocks = nullptr; uint32_t *key0 = nullptr, *key1 = nullptr, *val0 = nullptr, *val1 = nullptr;
  uint32_t *snext = nullptr, *ssteps = nullptr, *srank = nullptr, *resume = nullptr; int32_t* d_err = nullptr;
  uint8_t* seg = nullptr;      // ib_walk1's kept bytes: SEG_CAP per splitter
  RadixWork sw;
  int take(ShareScratch& g, const IbPlan& P) {
    const size_t nb = P.nb, keys = 4 * (size_t)P.M + 64, spl = 4 * nb * P.spl_stride;
    CJS_TRY(g.take((void**)&d_blocks, sizeof(IbBlock) * nb));
    CJS_TRY(g.take((void**)&key0, keys)); CJS_TRY(g.take((void**)&key1, keys));
    if (!P.strided) { CJS_TRY(g.take((void**)&val0, keys)); CJS_TRY(g.take((void**)&val1, keys)); }      // (strided: the keys carry the indices)
    CJS_TRY(g.take((void**)&snext, spl)); CJS_TRY(g.take((void**)&ssteps, spl)); CJS_TRY(g.take((void**)&srank, spl));
    CJS_TRY(g.take((void**)&d_err, 4 * nb));
    CJS_TRY(g.take((void**)&resume, spl));
    // (the first walk's kept bytes: without them -- one large block among very many tiny ones would ask for SEG_CAP x 14,066 bytes for
    // each -- the second walk does all the work, as it does for the sentinel form)
    const uint64_t seg_bytes = (uint64_t)nb * P.spl_stride * SEG_CAP;
    if (seg_bytes <= (8ull << 30) && g.take((void**)&seg, (size_t)seg_bytes) != 0) seg = nullptr;
    sw.hist_tiles = (uint32_t)P.T; sw.bintot_segs = P.strided ? P.nb : 1u;
    CJS_TRY(g.take((void**)&sw.hist, RadixWork::hist_words(P.T) * 4));
    return g.take((void**)&sw.bintot, 256 * 4 * (size_t)sw.bintot_segs);
  }
};

// The T vector: keys, the stable sort (strided: one pass, segment by segment, the index riding on the key), then slot j of a block
// holds (T[j] << 8) | tt[j] in *d_dbuf, the key buffer the sort is not sitting in.
static int sort_and_pack(hipStream_t s, IbScratch& q, const IbPlan& P, uint32_t** d_dbuf) {
  if (P.strided) hipLaunchKernelGGL(ib_make_keys_hist, dim3(P.tps, P.nb), dim3(256), 0, s, q.d_blocks, q.key0, P.seg_stride, P.tps, q.sw.hist);
  else hipLaunchKernelGGL(ib_make_keys, dim3(64, P.nb), dim3(256), 0, s, q.d_blocks, q.key0, q.val0, 0u);
  int cur = 0;
  // (whole digits are sorted: the rest of the last one is zero, ib_make_keys' (block << 8) | byte has block < nb on top)
  if (P.strided) CJS_TRY(radix_pass_segments(s, q.sw, q.key0, q.val0, q.key1, q.val1, cur, P.nb, P.seg_stride, 0, 8, true, true));
  else CJS_TRY(radix_passes<uint32_t>(s, q.sw, q.key0, q.val0, q.key1, q.val1, cur, P.M, 0, 8 + bits_for(P.nb - 1)));
  const uint32_t* sval = P.strided ? (cur ? q.key1 : q.key0) : (cur ? q.val1 : q.val0);
  *d_dbuf = cur ? q.key0 : q.key1;
  hipLaunchKernelGGL(ib_pack, dim3(64, P.nb), dim3(256), 0, s, q.d_blocks, sval, *d_dbuf, P.strided ? 1 : 0);
  return 0;
}
// walk to the next splitter, rank the splitters, put the kept bytes in their places, walk again for the rest; periodic blocks repeat
static void walks(hipStream_t s, const IbScratch& q, const IbPlan& P, const uint32_t* d_dbuf, uint8_t* d_wb) {
  const uint32_t nb = P.nb, cpb = walk_chunks(P.maxc), wgrid = ((nb * cpb + 7u) >> 3) << 3;
  hipLaunchKernelGGL(ib_walk1, dim3(wgrid), dim3(WALK_T), WALK_LDS, s, d_dbuf, q.d_blocks, nb, cpb, P.spl_stride, q.snext, q.ssteps, 0, q.seg, q.resume);
  hipLaunchKernelGGL(ib_rank, dim3(nb), dim3(1024), 0, s, q.d_blocks, nb, P.spl_stride, q.snext, q.ssteps, q.srank, q.d_err);
  // (placing inside the second walk, whose workgroups are few per CU, was no faster than the two launches: 0.49 vs 0.21 + 0.26 ms)
  if (q.seg) hipLaunchKernelGGL(ib_place, dim3((P.spl_stride + 255) / 256, nb), dim3(256), 0, s, q.d_blocks, P.spl_stride, q.srank, q.ssteps, q.seg, d_wb);
  hipLaunchKernelGGL(ib_walk2, dim3(wgrid), dim3(WALK_T), WALK_LDS, s, d_dbuf, q.d_blocks, nb, cpb, P.spl_stride, q.srank, q.ssteps, d_wb, 0, q.resume, q.seg);
  hipLaunchKernelGGL(ib_periodic_fill, dim3(32, nb), dim3(256), 0, s, q.d_blocks, q.d_err, d_wb);
}
// the blocks with their out_len and the walks' verdicts, with the stream drained
static int read_back(DecJob& J, DecShare& S, hipStream_t s, const IbScratch& q, size_t b0, std::vector<int32_t>& errs) {
  const size_t nb = errs.size();
  DEC_HIP(hipGetLastError());
  DEC_HIP(hipMemcpyAsync(J.chain.data() + b0, q.d_blocks, sizeof(IbBlock) * nb, hipMemcpyDeviceToHost, s));
  DEC_HIP(hipMemcpyAsync(errs.data(), q.d_err, 4 * nb, hipMemcpyDeviceToHost, s));
  DEC_HIP(hipStreamSynchronize(s));
  S.h2d += sizeof(IbBlock) * nb; S.d2h += (sizeof(IbBlock) + 4) * nb;
  return 0;
}

// one batch [b0, b1) of the share's chain blocks
static int ib_batch(DecJob& J, DecShare& S, size_t b0, size_t b1) {
  hipStream_t s = S.s;
  const uint32_t nb = (uint32_t)(b1 - b0);
  S.b_batches++;
  const IbPlan P = ib_plan(nb, RS_TILE, [&](uint32_t k) { return J.chain[b0 + k].count; });
  if (!P.fits()) return CJS_E_UNSUPPORTED;                           // a single block list beyond the batch limit cannot happen (count <= 900000)
  for (uint32_t k = 0; k < nb; k++) { J.chain[b0 + k].woff = P.woff[k]; J.chain[b0 + k].off = P.off[k]; }
  IbScratch q; ShareScratch g(&S);
  CJS_TRY(q.take(g, P));
  DEC_HIP(hipMemcpyAsync(q.d_blocks, J.chain.data() + b0, sizeof(IbBlock) * nb, hipMemcpyHostToDevice, s));
  DEC_HIP(hipMemsetAsync(q.d_err, 0, 4 * (size_t)nb, s));
  uint8_t* d_wb = S.d_w + S.ebase[b0 - S.c0];
  uint32_t* d_dbuf = nullptr;
  CJS_TRY(sort_and_pack(s, q, P, &d_dbuf));
  walks(s, q, P, d_dbuf, d_wb);
  launch_unrle1_lengths(s, d_wb, q.d_blocks, nb, S.d_carry + (size_t)(b0 - S.c0) * S.carry_tiles, S.carry_tiles);
  std::vector<int32_t> errs(nb);
  CJS_TRY(read_back(J, S, s, q, b0, errs));
  g.done();
  for (int32_t e : errs) if (e <= 0) return CJS_E_DATA_ERROR;      // cannot happen: the walk makes >= 1 step
  return 0;
}

static int phase_b(DecJob& J, DecShare& S) {
  DEC_HIP(hipSetDevice(S.device));
  const size_t nbk = S.c1 - S.c0;
  S.ebase.assign(nbk + 1, 0);
  for (size_t i = 0; i < nbk; i++) S.ebase[i + 1] = S.ebase[i] + J.chain[S.c0 + i].count;
  S.carry_tiles = (J.tt_stride + UR_TILE - 1) / UR_TILE;              // RLE1 state carried into every tile: written by phase B, read by phase C
  CJS_TRY(S.take((void**)&S.d_w, (size_t)S.ebase[nbk] + 64));
  CJS_TRY(S.take((void**)&S.d_carry, sizeof(RleCarry) * (size_t)nbk * S.carry_tiles));
  int rc = 0;
  for (size_t b0 = S.c0; b0 < S.c1 && !rc;) {
    const size_t b1 = dec_next_batch(&J, b0, S.c1);
    rc = ib_batch(J, S, b0, b1);
    b0 = b1;
  }
  if (S.d_tt) { S.drop(S.d_tt); S.d_tt = nullptr; }                   // (a one-batch share's rows; a failed batch ends here too)
  return rc;
}
void dec_phase_b(DecJob* J, DecShare* S) {
  if (S->c1 <= S->c0) return;
  const auto T0 = std::chrono::steady_clock::now();
  S->rc = phase_b(*J, *S);
  S->ms_b = ms_since(T0);
}

// ---------------------------------------------------------------- inverse sentinel BWT of a batch (used by BWTC.decompressFile)
// The same sequence as ib_batch with its own allocations, always back to back, ib_pack_sentinel, the walks' sentinel flag and
// nothing kept by the first walk (so no place / fill), and no RLE1.
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
  // (whole digits are sorted: the rest of the last one is zero, ib_make_keys' (block << 8) | byte has block < nb on top)
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
