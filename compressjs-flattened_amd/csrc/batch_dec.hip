// batch_dec.hip -- the device side of Bzip2.decompressFiles (cjs_bzip2_decompress_batch): the batch magic scan and the batch
// form of block decode's per-candidate kernels (bz_stage2.h).  Kept out of decode.hip's module so that the single-stream
// kernels there compile exactly as they do without a batch form beside them.  The host driver is in dec_batch.hip.
#include "decode_dev.h"
#include <algorithm>

namespace cjs {
// Batch form (cjs_bzip2_decompress_batch): input k is bytes [st[k], en[k]) of the group, st ascending.  A thread tests bytes of
// its own input only (none in the gaps between inputs), reads past that input's end as zero -- so no candidate straddles two
// inputs -- and records the input in pad.
__global__ __launch_bounds__(256) void bz_magic_scan_batch(const uint8_t* __restrict__ in, const uint32_t* __restrict__ st, const uint32_t* __restrict__ en,
                                                           uint32_t count, uint64_t byte0, uint64_t byte1, Cand* __restrict__ out, uint32_t cap,
                                                           uint32_t* __restrict__ ncand) {
  const uint64_t byte = byte0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (byte >= byte1) return;
  uint32_t lo = 0, hi = count;                   // the last input that starts at or in front of the byte (an empty input shares its start with the next)
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (st[mid] <= byte) lo = mid; else hi = mid; }
  const uint64_t n = en[lo];
  if (byte < st[lo] || byte + 6 > n) return;
  uint64_t w = 0;
  for (int i = 0; i < 7; i++) w = (w << 8) | (byte + i < n ? in[byte + i] : 0);
  for (int b = 0; b < 8; b++) {
    if (byte * 8 + b + 48 > n * 8) break;
    const uint64_t v = (w >> (8 - b)) & 0xFFFFFFFFFFFFull;
    if (v == MAGIC_BLOCK || v == MAGIC_END) {
      const uint32_t idx = atomicAdd(ncand, 1u);
      if (idx < cap) { out[idx].bit = byte * 8 + b; out[idx].kind = v == MAGIC_END; out[idx].pad = lo; }
    }
  }
}


#define BZ_BATCH 1
#include "bz_stage2.h"
#undef BZ_BATCH

void launch_magic_scan_batch(hipStream_t s, const uint8_t* d_in, const uint32_t* d_st, const uint32_t* d_en, uint32_t count, uint64_t bytes,
                             Cand* d_cand, uint32_t cap, uint32_t* d_count) {
  for (uint64_t b0 = 0; b0 < bytes; b0 += 1ull << 31) {                // (slabs: a grid may not exceed 2^32 threads)
    const uint64_t b1 = std::min<uint64_t>(bytes, b0 + (1ull << 31));
    hipLaunchKernelGGL(bz_magic_scan_batch, dim3((unsigned)((b1 - b0 + 255) / 256)), dim3(256), 0, s, d_in, d_st, d_en, count, b0, b1, d_cand, cap, d_count);
  }
}

void launch_block_decode_batch(hipStream_t s, const uint8_t* d_in, const uint32_t* d_cend, const uint32_t* d_cdsz, uint32_t* d_rlim, const Cand* d_cand, uint32_t nc, uint32_t rows, uint32_t dsz,
                               RowTab* d_tabs, uint8_t* d_sel, uint32_t* d_gstart, uint8_t* d_l0, BlockOut* d_bo, uint32_t r0, uint32_t group_tiles,
                               uint16_t* d_syms, uint32_t sym_stride, uint32_t sym_groups, uint8_t* d_ops, uint32_t* d_opoff, uint32_t ops_stride, uint32_t* d_nops) {
  hipLaunchKernelGGL(bz_chain_batch, dim3(nc), dim3(CH_T), 0, s, d_in, 0, d_cand, nc, dsz, d_tabs, d_sel, d_gstart, d_l0, d_bo, r0, d_cend, d_cdsz, d_rlim);
  if (rows) hipLaunchKernelGGL(bz_group_syms_batch, dim3(group_tiles, rows), dim3(256), 0, s, d_in, 0, d_tabs, d_sel, d_gstart, d_syms, sym_stride, sym_groups, 0u, d_rlim);
  hipLaunchKernelGGL(bz_sym_ops_batch, dim3(nc), dim3(1024), 0, s, d_tabs, d_cand, nc, d_syms, sym_groups, dsz, d_ops, d_opoff, ops_stride, d_nops, d_bo, r0, 0, d_cdsz);
}

}  // namespace cjs
