// rle1_bytes.hip — stage 0b: the RLE1 bytes of the blocks that the boundary walk (rle1.hip) found, and their CRCs (crc.hip).
#include "rle1_dev.hpp"
#include "rle1.h"
#include "crc.h"

namespace cjs {

// ---- R: materialise the RLE1 bytes of every block (grid = input tiles)
__global__ __launch_bounds__(256) void rle_materialize(const uint8_t* __restrict__ in, uint64_t N, uint32_t cap,
                                                       const uint64_t* __restrict__ run_start_in, const uint64_t* __restrict__ next_bnd,
                                                       const uint64_t* __restrict__ gt, const RleBlock* __restrict__ blocks,
                                                       const uint32_t* __restrict__ nblocks_p, uint32_t first, uint32_t count,
                                                       uint8_t* __restrict__ out) {
  __shared__ uint32_t smem[256 + 16];
  __shared__ uint32_t nb_first[256];
  const uint32_t nblocks = *nblocks_p < first + count ? *nblocks_p : first + count;   // blocks [first, nblocks)
  const uint64_t tile_start = (uint64_t)blockIdx.x * RT;
  if (nblocks <= first || tile_start >= blocks[nblocks - 1].e || tile_start + RT <= blocks[first].s) return;
  uint8_t b[16]; uint32_t bm; uint64_t rs;
  run_starts<256, 16>(in, N, tile_start, run_start_in[blockIdx.x], smem, b, bm, rs);
  const uint64_t p0 = tile_start + (uint64_t)threadIdx.x * 16;
  // global c and its exclusive prefix inside the tile
  uint32_t dpg[16];
  const uint32_t cnt = emit16(p0, N, rs, bm, dpg);
  uint32_t tot;
  const uint32_t exc = block_excl_sum<256>(cnt, smem, tot);
  // next boundary after each position: tile-relative first boundary per thread, exclusive suffix-min over threads
  const uint32_t myfirst = bm ? (uint32_t)threadIdx.x * 16u + (uint32_t)__builtin_ctz(bm) : 0xFFFFu;
  {
    const uint32_t q = 255 - threadIdx.x;                 // reversed thread order
    nb_first[q] = myfirst == 0xFFFFu ? 0u : 0x10000u - myfirst;
    __syncthreads();
    const uint32_t v = nb_first[threadIdx.x];
    const uint32_t im = block_incl_max<256>(v, smem);
    __syncthreads();
    nb_first[threadIdx.x] = im;
    __syncthreads();
  }
  const uint32_t rq = 255 - threadIdx.x;
  const uint32_t sfx = rq ? nb_first[rq - 1] : 0u;        // max over later threads of (0x10000 - first)
  const uint64_t next_after_me = sfx ? tile_start + (0x10000u - sfx) : next_bnd[blockIdx.x];
  // blocks overlapping this tile: first block with e > tile_start
  uint32_t lo = first, hi = nblocks - 1;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (blocks[mid].e > tile_start) hi = mid; else lo = mid + 1; }
  const uint64_t tile_end = tile_start + RT;
  {
    // A tile strictly inside one block, behind the block's re-chunked first run: its output is one contiguous byte range
    // of the block.  It is put together in LDS and written with aligned 32-bit stores (the general path below stores byte
    // by byte, sixteen scattered bytes per lane: 0.26 ms per 100 MB, most of it waiting for partial-line writes).
    __shared__ __attribute__((aligned(16))) uint8_t stage[RT + RT / 4 + 64];
    const RleBlock bd = blocks[lo];
    const uint64_t off0 = (uint64_t)bd.base + (gt[blockIdx.x] - bd.Gr);
    const bool fast = tile_start >= bd.s && tile_start >= bd.r_end && tile_end < bd.e && tile_end <= N && off0 + tot + 1 < cap;
    if (fast) {
      uint32_t run = exc;
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const uint32_t dp = dpg[j];
        if (dp < 4) {
          stage[run] = b[j];
          if (dp == 3) {
            uint64_t re = next_after_me;               // run end = next boundary after p
            const uint32_t later = (j < 15) ? (bm >> (j + 1)) : 0u;
            if (later) re = p0 + j + 1 + (uint32_t)__builtin_ctz(later);
            uint64_t follow = re - (p0 + j + 1);
            if (follow > 251) follow = 251;
            stage[run + 1] = (uint8_t)follow;
          }
        }
        run += chunk_emit(dp);
      }
      __syncthreads();
      uint8_t* dst = out + (size_t)(lo - first) * cap + off0;
      const uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u) < tot ? (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u) : tot;
      const uint32_t n4 = (tot - head) >> 2, tail0 = head + 4u * n4;
      if (threadIdx.x < head) dst[threadIdx.x] = stage[threadIdx.x];
      const uint32_t* st32 = reinterpret_cast<const uint32_t*>(stage);
      uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + head);
      for (uint32_t i = threadIdx.x; i < n4; i += 256) {
        const uint32_t sb = head + 4u * i, w0 = st32[sb >> 2], w1 = st32[(sb >> 2) + 1];
        d32[i] = __builtin_amdgcn_alignbyte(w1, w0, sb & 3u);
      }
      if (threadIdx.x < tot - tail0) dst[tail0 + threadIdx.x] = stage[tail0 + threadIdx.x];
      return;
    }
  }
  for (uint32_t k = lo; k < nblocks; k++) {
    const RleBlock bd = blocks[k];
    if (bd.s >= tile_end) break;
    uint8_t* o = out + (size_t)(k - first) * cap;
    uint32_t run = exc;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t p = p0 + j;
      const uint32_t cg = chunk_emit(dpg[j]);
      if (p < N && p >= bd.s && p < bd.e) {
        uint32_t dp; uint64_t off;
        if (p < bd.r_end) { const uint64_t d = p - bd.s; dp = (uint32_t)(d % 255); off = fresh_offset(d); }
        else { dp = dpg[j]; off = (uint64_t)bd.base + (gt[blockIdx.x] + run - bd.Gr); }
        if (dp < 4 && off < cap) {
          o[off] = b[j];
          if (dp == 3 && off + 1 < cap) {
            // run end = next boundary after p
            uint64_t re = next_after_me;
            const uint32_t later = (j < 15) ? (bm >> (j + 1)) : 0u;
            if (later) re = p + 1 + (uint32_t)__builtin_ctz(later);
            uint64_t follow = re - (p + 1);
            if (follow > 251) follow = 251;
            if (off + 2 == cap) follow = 0;                    // count byte fills the block: stays 0 (Q2)
            o[off + 1] = (uint8_t)follow;
          }
        }
      }
      run += (p < N) ? cg : 0u;                                  // (cg is 0 behind N as it is; without the select: 16 more VGPRs)
    }
  }
}

// Stage 0b: RLE1 bytes (d_blocks, block k at (k-first)*cap) and CRCs (block_crc[k], absolute) of blocks [first, first+count)
int rle1_finish(hipStream_t s, Rle1Work& w, const uint8_t* d_in, uint64_t N, uint32_t first, uint32_t count, uint8_t* d_blocks,
                hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join) {
  if (N == 0 || count == 0) return 0;
  if (count > w.range_blocks) return CJS_E_INVALID_ARG;
  const uint32_t Tn = tiles_for(N);
  // the block CRCs read only the input and the block table: with a side stream they run beside the suffix sort
  // (ev_join is recorded at their end; the caller makes the packing stage wait for it)
  hipStream_t cs = s;
  if (side) {
    CJS_HIP_TRY(hipEventRecord(ev_fork, s));
    CJS_HIP_TRY(hipStreamWaitEvent(side, ev_fork, 0));
    cs = side;
  }
  hipLaunchKernelGGL(rle_materialize, dim3(Tn), dim3(256), 0, s, d_in, N, w.cap, w.lb, w.fb, w.gt, w.blocks, w.nblocks, first, count, d_blocks);
  CJS_HIP_TRY(hipGetLastError());
  CJS_TRY(crc_ranges_at(cs, d_in, w.blocks, w.nblocks, first, count, w.max_segs, w.seg_crc, w.block_crc));
  if (side) CJS_HIP_TRY(hipEventRecord(ev_join, side));
  return 0;
}

}  // namespace cjs
