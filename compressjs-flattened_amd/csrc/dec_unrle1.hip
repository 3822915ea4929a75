// dec_unrle1.hip — steps 5 and 6 of the Bzip2 decoder (the map: decode.hip): the RLE1 expansion kernels, their length launches
// for phase B, and phase C of the engine (dec_engine.h): expansion to the final offsets, block CRCs, D2H.
#include "dec_engine.h"
#include "prims.hpp"
#include "crc.h"

using namespace cjs;

namespace cjs {

// ---------------------------------------------------------------- 5. RLE1 expansion
// Stretch functions on the carried bit c0 ("this stretch starts with a count byte"): next = ((L - c0) % 5 == 4)
//   L % 5 == 4 -> NOT-ish (c0=0 ->1, c0=1 -> 0), L % 5 == 0 -> identity, else const 0.  Encoded as 2 bits (f(0) | f(1) << 1).
__device__ __forceinline__ uint32_t stretch_fn(uint32_t L) { const uint32_t m = L % 5; return m == 4 ? 1u : (m == 0 ? 2u : 0u); }
__device__ __forceinline__ uint32_t fn_apply(uint32_t f, uint32_t c) { return (f >> c) & 1u; }
__device__ __forceinline__ uint32_t fn_compose(uint32_t first, uint32_t then) {     // x -> then(first(x))
  return fn_apply(then, fn_apply(first, 0)) | (fn_apply(then, fn_apply(first, 1)) << 1);
}
// One tile (UR_TILE = 1024 threads x UR_BPT bytes, decode_dev.h) of a block by one workgroup.  Carried from the tiles in front (RleCarry): start of the
// current stretch, c0 of the current stretch, output bytes so far (from the length pass below); the bytes go out.
constexpr int UR_BPT_C = UR_BPT;
static_assert(UR_BPT_C == 16, "ur_load");
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

// ---------------------------------------------------------------- the length pass, for phase B
void launch_unrle1_lengths(hipStream_t s, const uint8_t* d_w, IbBlock* d_blocks, uint32_t nb, RleCarry* d_carry, uint32_t carry_tiles) {
  hipLaunchKernelGGL(unrle1_bounds, dim3(carry_tiles, nb), dim3(1024), 0, s, d_w, d_blocks, d_carry, carry_tiles);
  hipLaunchKernelGGL(unrle1_sums, dim3(carry_tiles, nb), dim3(1024), 0, s, d_w, d_blocks, d_carry, carry_tiles);
  hipLaunchKernelGGL(unrle1_carries, dim3(nb), dim3(64), 0, s, d_blocks, d_carry, carry_tiles);
}

// Bad block CRC (:1756-1761): the detail text
void bad_crc_detail(char* d, size_t cap, uint32_t got, uint32_t expected) { snprintf(d, cap, "Bad block CRC (got %x expected %x)", got, expected); }

// ---------------------------------------------------------------- phase C: RLE1 expansion to the final byte offsets, block CRC check, D2H
// One inverse-BWT batch [b0, b0 + nb) of the share's chain blocks as phase C sees it
struct CBatch {
  size_t b0; uint32_t nb;
  uint64_t e0, o0, obytes;            // the batch's first byte in S.d_w / in the output, its output bytes
  std::vector<IbBlock> blk;           // the blocks with offsets local to the batch
  uint32_t need_segs = 1;             // CRC segments of its longest block
  IbBlock* d_blocks = nullptr; uint8_t* d_out = nullptr; RleBlock* d_ranges = nullptr; uint32_t *d_nb = nullptr, *d_seg = nullptr, *d_crc = nullptr;
};

// the batch-local block list and need_segs
static CBatch c_batch(const DecJob& J, const DecShare& S, size_t b0, size_t b1) {
  CBatch B{b0, (uint32_t)(b1 - b0), S.ebase[b0 - S.c0], J.out_off[b0], J.out_off[b1] - J.out_off[b0], std::vector<IbBlock>(J.chain.begin() + (long)b0, J.chain.begin() + (long)b1)};
  for (uint32_t k = 0; k < B.nb; k++) {
    B.blk[k].off = B.blk[k].woff = (uint32_t)(S.ebase[b0 + k - S.c0] - B.e0);
    B.blk[k].out_off = J.out_off[b0 + k] - B.o0;                  // inside the batch's output buffer
    B.need_segs = std::max(B.need_segs, (uint32_t)crc_segs_for(B.blk[k].out_len));
  }
  return B;
}
// (a device sink: unrle1_write stores only inside [out_off, out_off + out_len) of each block, crc_ranges reads aligned 16-byte
// pieces that hold a byte of the range: the caller's buffer takes the bytes at their final offsets)
static int c_scratch(const DecJob& J, ShareScratch& g, CBatch& B) {
  B.d_out = J.dev_out ? J.dev_out + B.o0 : nullptr;
  CJS_TRY(g.take((void**)&B.d_blocks, sizeof(IbBlock) * B.nb));
  if (!J.dev_out) CJS_TRY(g.take((void**)&B.d_out, (size_t)B.obytes + 64));
  CJS_TRY(g.take((void**)&B.d_ranges, sizeof(RleBlock) * B.nb));
  CJS_TRY(g.take((void**)&B.d_nb, 64));
  CJS_TRY(g.take((void**)&B.d_seg, 4 * (size_t)B.nb * B.need_segs));
  return g.take((void**)&B.d_crc, 4 * (size_t)B.nb);
}
static int c_expand_and_crc(const DecShare& S, hipStream_t s, const CBatch& B) {
  DEC_HIP(hipMemcpyAsync(B.d_blocks, B.blk.data(), sizeof(IbBlock) * B.nb, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(unrle1_write, dim3(S.carry_tiles, B.nb), dim3(1024), 0, s, S.d_w + B.e0, B.d_blocks, S.d_carry + (size_t)(B.b0 - S.c0) * S.carry_tiles, S.carry_tiles, B.d_out);
  hipLaunchKernelGGL(ib_make_crc_ranges, dim3((B.nb + 63) / 64), dim3(64), 0, s, B.d_blocks, B.nb, B.d_ranges, B.d_nb);
  return crc_ranges(s, B.d_out, B.d_ranges, B.d_nb, B.nb, B.need_segs, B.d_seg, B.d_crc);
}
// the CRCs, and the bytes of a host sink, with the stream drained
static int c_copies(const DecJob& J, DecShare& S, hipStream_t s, const CBatch& B, std::vector<uint32_t>& crcs) {
  DEC_HIP(hipMemcpyAsync(crcs.data(), B.d_crc, 4 * (size_t)B.nb, hipMemcpyDeviceToHost, s));
  if (J.host && B.obytes) DEC_HIP(hipMemcpyAsync(J.host + B.o0, B.d_out, (size_t)B.obytes, hipMemcpyDeviceToHost, s));
  DEC_HIP(hipStreamSynchronize(s));
  S.h2d += sizeof(IbBlock) * (size_t)B.nb; S.d2h += 4 * (size_t)B.nb + (J.host ? (size_t)B.obytes : 0);
  return 0;
}
// batch mode: every block's CRC for the caller's verdicts; else the first bad one ends the call (:1756-1761)
static int c_verdict(DecJob& J, DecShare& S, const CBatch& B, const std::vector<uint32_t>& crcs) {
  if (J.batch) { for (uint32_t k = 0; k < B.nb; k++) J.crc_got[B.b0 + k] = crcs[k]; return 0; }      // (each input's verdict: the batch's host side)
  for (uint32_t k = 0; k < B.nb; k++) if (crcs[k] != B.blk[k].crc) {
    bad_crc_detail(S.detail, sizeof S.detail, crcs[k], B.blk[k].crc);
    if (env_debug()) fprintf(stderr, "[cjs dec] block %zu: Bad block CRC (got %08x expected %08x) out_len %u\n", B.b0 + k, crcs[k], B.blk[k].crc, B.blk[k].out_len);
    return CJS_E_DATA_ERROR;
  }
  return 0;
}

static int phase_c(DecJob& J, DecShare& S) {
  DEC_HIP(hipSetDevice(S.device));
  hipStream_t s = S.s;
  for (size_t b0 = S.c0; b0 < S.c1;) {
    const size_t b1 = dec_next_batch(&J, b0, S.c1);
    CBatch B = c_batch(J, S, b0, b1);
    ShareScratch g(&S);
    CJS_TRY(c_scratch(J, g, B));
    CJS_TRY(c_expand_and_crc(S, s, B));
    std::vector<uint32_t> crcs(B.nb);
    CJS_TRY(c_copies(J, S, s, B, crcs));
    const int rc = c_verdict(J, S, B, crcs);
    g.done();                                                       // (the stream has drained; a bad CRC ends the call all the same)
    if (rc) return rc;
    b0 = b1;
  }
  return 0;
}
void dec_phase_c(DecJob* J, DecShare* S) {
  if (S->c1 <= S->c0) return;
  const auto T0 = std::chrono::steady_clock::now();
  S->rc = phase_c(*J, *S);
  S->ms_c = ms_since(T0);
}

}  // namespace cjs
