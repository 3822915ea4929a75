// crc.hip — bzip2 CRC-32 of byte ranges on the GPU (the arithmetic: crc32_bz.h).  Every thread takes 64 bytes, multiplies its
// CRC0 by x^(8 * bytes behind its piece) and the workgroup XORs the products (rle_crc_partial: one word per window of a range);
// one thread per range then combines the windows (rle_crc_final).  The powers come from tables built at compile time.
#include "cjs_internal.h"
#include "crc.h"

namespace cjs {

__device__ const CrcTables g_crc_tables = make_crc_tables();

__global__ __launch_bounds__(256) void rle_crc_partial(const uint8_t* __restrict__ in, const RleBlock* __restrict__ blocks,
                                                       const uint32_t* __restrict__ nblocks_p, uint32_t max_segs,
                                                       uint32_t first, uint32_t* __restrict__ seg_crc) {
  __shared__ uint32_t tab[4][256];
  __shared__ uint32_t pw64[256], px[64];
  __shared__ uint32_t seg[CRC_SEG / 4 + CRC_SEG / 64];      // dword d of the window lives at d + d/16 (bank-conflict-free 64-byte strides)
  __shared__ uint32_t part[4];
  const uint32_t k = first + blockIdx.y;
  if (k >= *nblocks_p) return;
  const RleBlock bd = blocks[k];
  const int tid = threadIdx.x;
  // absolute byte addresses; windows are aligned in the address space so that every staging load is a 16-byte aligned one
  const uint64_t A0 = (uint64_t)(uintptr_t)in, S = A0 + bd.s, E = A0 + bd.e;
  if (crc_window(S, E, blockIdx.x).W >= E) return;
  for (int j = 0; j < 4; j++) tab[j][tid] = g_crc_tables.tab[j][tid];
  pw64[tid] = g_crc_tables.pw64[tid];
  if (tid < 64) px[tid] = g_crc_tables.px[tid];
  for (uint32_t sgi = blockIdx.x; crc_window(S, E, sgi).W < E; sgi += gridDim.x) {
    const CrcWindow w = crc_window(S, E, sgi);
    const uint64_t W = w.W, lo = w.lo, hi = w.hi;              // bytes of the block in this window
    __syncthreads();
    for (int j = 0; j < 4; j++) {
      const uint32_t c = (uint32_t)j * 256u + tid;                 // 16-byte chunk of the window
      const uint64_t ca = W + (uint64_t)c * 16;
      if (ca + 16 > lo && ca < hi) {
        const uint4 v = *(const uint4*)(uintptr_t)ca;              // may include bytes outside [lo,hi): never used
        const uint32_t d = c * 4u, o = d + (d >> 4);
        seg[o] = v.x; seg[o + 1] = v.y; seg[o + 2] = v.z; seg[o + 3] = v.w;
      }
    }
    __syncthreads();
    const uint64_t ca = W + (uint64_t)tid * 64, cb = ca + 64;
    const uint64_t a = ca > lo ? ca : lo, b = cb < hi ? cb : hi;
    uint32_t crc = 0;
    if (a < b) {
      const uint32_t o = (uint32_t)tid * 17u;
      if (b - a == 64) {
#pragma unroll 4
        for (int i = 0; i < 16; i++) {
          const uint32_t x = crc ^ __builtin_bswap32(seg[o + i]);
          crc = tab[3][x >> 24] ^ tab[2][(x >> 16) & 0xff] ^ tab[1][(x >> 8) & 0xff] ^ tab[0][x & 0xff];
        }
      } else {
        for (uint64_t p = a; p < b; p++) {
          const uint32_t off = (uint32_t)(p - ca);
          const uint32_t byte = (seg[o + (off >> 2)] >> (8u * (off & 3u))) & 0xffu;
          crc = (crc << 8) ^ tab[0][((crc >> 24) ^ byte) & 0xff];
        }
      }
      const uint32_t behind = (uint32_t)(hi - b);
      if (behind) crc = gf_mul(crc, gf_xpow8_small(behind, pw64, px));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) crc ^= __shfl_xor(crc, m, 64);
    if ((tid & 63) == 0) part[tid >> 6] = crc;
    __syncthreads();
    if (tid == 0) seg_crc[(size_t)blockIdx.y * max_segs + sgi] = part[0] ^ part[1] ^ part[2] ^ part[3];
  }
}

__global__ void rle_crc_final(const RleBlock* __restrict__ blocks, const uint32_t* __restrict__ nblocks_p, uint32_t max_segs,
                              uint32_t first, uint32_t count, const uint8_t* __restrict__ in, const uint32_t* __restrict__ seg_crc,
                              uint32_t* __restrict__ block_crc) {
  const uint32_t rel = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t k = first + rel;
  if (rel >= count || k >= *nblocks_p) return;
  const RleBlock bd = blocks[k];
  const uint64_t n = bd.e - bd.s;
  const uint64_t A0 = (uint64_t)(uintptr_t)in, S = A0 + bd.s, E = A0 + bd.e;
  const uint32_t xfull = gf_mul(g_crc_tables.pw64[255], g_crc_tables.pw64[1]);     // x^(8*16384)
  uint32_t crc = 0;
  for (uint32_t sgi = 0; crc_window(S, E, sgi).W < E; sgi++) {
    const CrcWindow w = crc_window(S, E, sgi);
    const uint32_t l = (uint32_t)(w.hi - w.lo);
    crc = gf_mul(crc, l == CRC_SEG ? xfull : gf_xpow8_small(l, g_crc_tables.pw64, g_crc_tables.px)) ^ seg_crc[(size_t)rel * max_segs + sgi];
  }
  crc ^= gf_mul(0xFFFFFFFFu, gf_xpow8(n));     // init = ~0 carried through n bytes
  block_crc[k] = ~crc;
}

int crc_ranges_at(hipStream_t s, const uint8_t* d_data, const RleBlock* d_blocks, const uint32_t* d_nblocks, uint32_t first, uint32_t count,
                  uint32_t max_segs, uint32_t* d_seg_crc, uint32_t* d_crc_out) {
  if (!count) return 0;
  hipLaunchKernelGGL(rle_crc_partial, dim3(64, count), dim3(256), 0, s, d_data, d_blocks, d_nblocks, max_segs, first, d_seg_crc);
  hipLaunchKernelGGL(rle_crc_final, dim3((count + 63) / 64), dim3(64), 0, s, d_blocks, d_nblocks, max_segs, first, count, d_data, d_seg_crc, d_crc_out);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}
// CRC-32 of arbitrary byte ranges [s,e) of d_data (used by the decoder for the per-block output CRCs)
int crc_ranges(hipStream_t s, const uint8_t* d_data, const RleBlock* d_blocks, const uint32_t* d_nblocks, uint32_t count, uint32_t max_segs,
               uint32_t* d_seg_crc, uint32_t* d_crc_out) {
  return crc_ranges_at(s, d_data, d_blocks, d_nblocks, 0u, count, max_segs, d_seg_crc, d_crc_out);
}

}  // namespace cjs
