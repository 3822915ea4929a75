// rle1_dev.hpp — device helpers shared by the stage-0 kernels (rle1.hip, rle1_bytes.hip, rle1_batch.hip): a lane's 16 input
// bytes, their run boundaries, the run start carried into a lane, and the bytes the lane emits under the chunk rule.
#pragma once
#include "cjs_internal.h"
#include "prims.hpp"
#include "rle1_rules.h"

namespace cjs {

constexpr uint64_t NONE64 = ~0ull;

// 16 consecutive input bytes of one lane as ONE 16-byte load when the address allows it (consecutive lanes then read
// consecutive 16-byte words: a wave covers 1 KiB per instruction instead of touching 16 lines sixteen times)
__device__ __forceinline__ void load16(const uint8_t* __restrict__ in, uint64_t N, uint64_t p0, uint8_t (&b)[16]) {
  if (p0 + 16 <= N && (((uintptr_t)(in + p0)) & 15u) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(in + p0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; j++) b[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  } else {
#pragma unroll
    for (int j = 0; j < 16; j++) b[j] = p0 + j < N ? in[p0 + j] : 0;
  }
}

// The run-boundary loop of one lane: loads the 16 bytes at p0 (0 behind N) and returns their boundary flags, bit j set when
// position p0 + j < end starts a run (it is position 0, or its byte differs from the one in front of it).  end <= N.
// last = (index of the last flag) + 1, 0 = none; the first flag is ctz of the flags.
__device__ __forceinline__ uint32_t boundaries16(const uint8_t* __restrict__ in, uint64_t N, uint64_t p0, uint64_t end, uint8_t (&b)[16], uint32_t& last) {
  uint8_t prev = 0;
  if (p0 > 0 && p0 - 1 < N) prev = in[p0 - 1];
  load16(in, N, p0, b);
  uint32_t bmask = 0;
  last = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint64_t p = p0 + j;
    if (p < end && (p == 0 || b[j] != prev)) { bmask |= 1u << j; last = (uint32_t)j + 1u; }
    prev = b[j];
  }
  return bmask;
}

// Per-thread view of ITEMS consecutive positions starting at p0: boundary flags and the run start
// governing the first position.  BLOCK threads cover BLOCK*ITEMS positions from tile_start.
// carry = start of the run that contains tile_start when tile_start itself is not a boundary.
// Leaves (the tile's last boundary, tile-relative) + 1, 0 = none, in smem[16 + BLOCK - 1].
// (The boundary loop stands here a second time: through boundaries16 the kernels that call this take up to 27 more VGPRs.)
template <int BLOCK, int ITEMS>
__device__ __forceinline__ void run_starts(const uint8_t* __restrict__ in, uint64_t N, uint64_t tile_start, uint64_t carry,
                                           uint32_t* smem /* BLOCK + 16 u32 */, uint8_t (&b)[ITEMS], uint32_t& bmask, uint64_t& rs_first) {
  const uint64_t p0 = tile_start + (uint64_t)threadIdx.x * ITEMS;
  uint8_t prev = 0;
  if (p0 > 0 && p0 - 1 < N) prev = in[p0 - 1];
  bmask = 0;
  uint32_t last = 0;     // (tile-relative index of my last boundary)+1
  if (ITEMS == 16) load16(in, N, p0, reinterpret_cast<uint8_t (&)[16]>(b));
  else {
#pragma unroll
    for (int j = 0; j < ITEMS; j++) b[j] = p0 + j < N ? in[p0 + j] : 0;
  }
#pragma unroll
  for (int j = 0; j < ITEMS; j++) {
    const uint64_t p = p0 + j;
    const bool bd = p < N && (p == 0 || b[j] != prev);
    if (bd) { bmask |= 1u << j; last = (uint32_t)(p - tile_start) + 1u; }
    prev = b[j];
  }
  const uint32_t im = block_incl_max<BLOCK>(last, smem);
  smem[16 + threadIdx.x] = im;
  __syncthreads();
  const uint32_t ex = threadIdx.x ? smem[16 + threadIdx.x - 1] : 0u;
  __syncthreads();
  rs_first = ex ? tile_start + ex - 1 : carry;
}

// Emission of the 16 bytes of this thread under the chunk rule, counted from the run start rs of the first byte and from the
// boundaries bm behind it: dpv[j] = offset in the chunk (255: past the end, emits nothing), returns the bytes emitted
__device__ __forceinline__ uint32_t emit16(uint64_t p0, uint64_t N, uint64_t rs, uint32_t bm, uint32_t (&dpv)[16]) {
  uint32_t dp = p0 < N ? (uint32_t)((p0 - rs) % 255) : 0u, cnt = 0;      // offset in the run mod 255: one 64-bit remainder per thread, then +1 per byte
#pragma unroll
  for (int j = 0; j < 16; j++) {
    dpv[j] = 255;
    if (p0 + j < N) {
      if ((bm >> j) & 1u) dp = 0;
      dpv[j] = dp;
      cnt += chunk_emit(dp);
      dp = chunk_next(dp);
    }
  }
  return cnt;
}

}  // namespace cjs
