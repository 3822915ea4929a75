// rle1_batch.hip — stage 0 for batches of independent inputs (cjs_bzip2_compress_batch*): input k = in[se[2k] .. se[2k+1]).
// One workgroup per input walks its 4 KiB tiles in order and carries the run start and the emitted count from tile to tile, so
// runs and the 255-chunking restart at every input (an input that starts with the previous input's last byte does not continue
// its run), and no tile table straddles two inputs.
#include "rle1_dev.hpp"
#include "rle1.h"

namespace cjs {

// RLE1 length of every input (fresh chunking from its first byte), counted until it passes `cap`:
// out[k] = min(len, cap + 1) << 1 | (the input's last byte is absorbed into a run-length byte)
// The reference ends a block as soon as `cap` bytes are out (J/Bzip2_joined_.js:1958-1961), so an input is ONE block iff
// len < cap, or len == cap and its last byte emits (no absorbed bytes left behind the full block).
__global__ __launch_bounds__(256) void rle_batch_len(const uint8_t* __restrict__ in_all, const uint64_t* __restrict__ se, uint32_t cap,
                                                     uint64_t* __restrict__ out) {
  __shared__ uint32_t smem[256 + 16];
  const uint32_t k = blockIdx.x;
  const uint8_t* in = in_all + se[2 * k];
  const uint64_t N = se[2 * k + 1] - se[2 * k];
  uint64_t carry = 0, E = 0;
  uint32_t absorbed = 0;
  for (uint64_t t0 = 0; t0 < N; t0 += RT) {
    uint8_t b[16]; uint32_t bm; uint64_t rs;
    run_starts<256, 16>(in, N, t0, carry, smem, b, bm, rs);
    const uint32_t tlast = smem[16 + 255];              // (last boundary of the tile) + 1, tile-relative; 0 = none
    const uint64_t p0 = t0 + (uint64_t)threadIdx.x * 16;
    uint32_t dpv[16];
    const uint32_t cnt = emit16(p0, N, rs, bm, dpv);
#pragma unroll
    for (int j = 0; j < 16; j++) if (p0 + j + 1 == N) absorbed = dpv[j] >= 4;
    uint32_t tot;
    (void)block_excl_sum<256>(cnt, smem, tot);
    E += tot;
    carry = tlast ? t0 + tlast - 1 : carry;
    if (E > cap) break;                                  // (uniform: every thread has the same E)
  }
  absorbed = block_sum<256>(absorbed, smem);
  if (threadIdx.x == 0) out[k] = ((E > cap ? (uint64_t)cap + 1 : E) << 1) | (absorbed ? 1u : 0u);
}

// Block boundaries of inputs of more than one block: one workgroup per input (item[j]) walks it block after block.  A block starts
// with fresh chunking at its first byte and ends with the first byte whose output reaches `cap` bytes (the reference
// stops at that point, even between a fourth equal byte and its run-length byte, J/Bzip2_joined_.js:1958-1961); the last block
// ends with the input.  Blocks of item j go to out[tbase[j] ..] (at most tbase[j+1] - tbase[j]; s / e relative to the input,
// len = RLE1 bytes), their number to nblk[j].
__global__ __launch_bounds__(256) void rle_batch_walk(const uint8_t* __restrict__ in_all, const uint64_t* __restrict__ se,
                                                      const uint32_t* __restrict__ item, const uint32_t* __restrict__ tbase, uint32_t cap,
                                                      RleBlock* __restrict__ out, uint32_t* __restrict__ nblk) {
  __shared__ uint32_t smem[256 + 16];
  __shared__ uint32_t s_end;
  const uint32_t k = item[blockIdx.x];
  const uint8_t* in = in_all + se[2 * k];
  const uint64_t N = se[2 * k + 1] - se[2 * k];
  const uint32_t tcap = tbase[blockIdx.x + 1] - tbase[blockIdx.x];
  RleBlock* ob = out + tbase[blockIdx.x];
  uint32_t nb = 0;
  for (uint64_t s = 0; s < N;) {
    const uint8_t* bin = in + s;
    const uint64_t BN = N - s;
    uint64_t carry = 0, e = BN;
    uint32_t E = 0, len = 0;
    bool full = false;
    for (uint64_t t0 = 0; t0 < BN; t0 += RT) {
      uint8_t b[16]; uint32_t bm; uint64_t rs;
      run_starts<256, 16>(bin, BN, t0, carry, smem, b, bm, rs);
      const uint32_t tlast = smem[16 + 255];
      const uint64_t p0 = t0 + (uint64_t)threadIdx.x * 16;
      uint32_t dpv[16];
      const uint32_t cnt = emit16(p0, BN, rs, bm, dpv);
      uint32_t tot;
      const uint32_t ex = block_excl_sum<256>(cnt, smem, tot);
      if (E + tot >= cap) {                              // the block ends in this tile (uniform)
        if (threadIdx.x == 0) s_end = 0xFFFFFFFFu;
        __syncthreads();
        uint32_t g = E + ex;
#pragma unroll
        for (int j = 0; j < 16; j++) {
          const uint32_t c = chunk_emit(dpv[j]);
          if (c && g < cap && g + c >= cap) atomicMin(&s_end, (uint32_t)threadIdx.x * 16u + (uint32_t)j);
          g += c;
        }
        __syncthreads();
        e = t0 + s_end + 1; len = cap; full = true;
        break;
      }
      E += tot;
      carry = tlast ? t0 + tlast - 1 : carry;
    }
    if (!full) len = E;
    if (threadIdx.x == 0 && nb < tcap) { RleBlock r{}; r.s = s; r.e = s + e; r.len = len; ob[nb] = r; }
    nb++;
    s += e;
    __syncthreads();                                     // (s_end is read by every thread before the next block sets it)
  }
  if (threadIdx.x == 0) nblk[blockIdx.x] = nb;
}

// RLE1 bytes of block j = in[blk[j].s .. blk[j].e) with fresh chunking, its first blk[j].len bytes written to out[j*stride ..].
// Literal bytes go to their prefix position; the byte that ends a chunk of >= 4 equal bytes writes the chunk's run-length byte
// (a block cut between a fourth equal byte and its run-length byte leaves that byte out: it lies at len).
__global__ __launch_bounds__(256) void rle_batch_materialize(const uint8_t* __restrict__ in_all, const RleBlock* __restrict__ blk,
                                                             uint32_t stride, uint8_t* __restrict__ out) {
  __shared__ uint32_t smem[256 + 16];
  const RleBlock bd = blk[blockIdx.x];
  const uint8_t* in = in_all + bd.s;
  const uint64_t N = bd.e - bd.s;
  const uint32_t L = bd.len;
  uint8_t* o = out + (size_t)blockIdx.x * stride;
  uint64_t carry = 0;
  uint32_t E = 0;
  for (uint64_t t0 = 0; t0 < N; t0 += RT) {
    uint8_t b[16]; uint32_t bm; uint64_t rs;
    run_starts<256, 16>(in, N, t0, carry, smem, b, bm, rs);
    const uint32_t tlast = smem[16 + 255];
    const uint64_t p0 = t0 + (uint64_t)threadIdx.x * 16;
    const uint32_t nxt = p0 + 16 < N ? in[p0 + 16] : 0x100u;   // the byte behind this thread's sixteen (none: 0x100)
    uint32_t dpv[16];
    const uint32_t cnt = emit16(p0, N, rs, bm, dpv);
    uint32_t tot;
    uint32_t g = E + block_excl_sum<256>(cnt, smem, tot);
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t p = p0 + j;
      if (p < N) {
        const uint32_t d = dpv[j];
        if (d < 4 && g < L) o[g] = b[j];
        const uint32_t next = j < 15 ? (p + 1 < N ? (uint32_t)b[j + 1] : 0x100u) : nxt;
        if (d >= 3 && (next != b[j] || d == 254)) {      // chunk ends here
          const uint32_t q = d == 3 ? g + 1 : g - 1;
          if (q < L) o[q] = (uint8_t)(d - 3);
        }
        g += chunk_emit(d);
      }
    }
    E += tot;
    carry = tlast ? t0 + tlast - 1 : carry;
  }
}

int rle1_batch_len(hipStream_t s, const uint8_t* d_in, const uint64_t* d_se, uint32_t count, uint32_t cap, uint64_t* d_len2) {
  if (!count) return 0;
  hipLaunchKernelGGL(rle_batch_len, dim3(count), dim3(256), 0, s, d_in, d_se, cap, d_len2);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}
int rle1_batch_walk(hipStream_t s, const uint8_t* d_in, const uint64_t* d_se, const uint32_t* d_item, const uint32_t* d_tbase, uint32_t count,
                    uint32_t cap, RleBlock* d_blocks, uint32_t* d_nblk) {
  if (!count) return 0;
  hipLaunchKernelGGL(rle_batch_walk, dim3(count), dim3(256), 0, s, d_in, d_se, d_item, d_tbase, cap, d_blocks, d_nblk);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}
int rle1_batch_materialize(hipStream_t s, const uint8_t* d_in, const RleBlock* d_blk, uint32_t nb, uint32_t stride, uint8_t* d_blocks) {
  if (!nb) return 0;
  hipLaunchKernelGGL(rle_batch_materialize, dim3(nb), dim3(256), 0, s, d_in, d_blk, stride, d_blocks);
  CJS_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace cjs
