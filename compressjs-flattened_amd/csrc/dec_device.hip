// dec_device.hip -- the kernels of the device-resident Bzip2 decode (cjs_bzip2_decompress_device, dec_batch.hip): what the host path
// reads of its host copy of the input, read on the device.  Only metadata crosses PCIe:
//   dd_headers     the first 4 bytes of every input (_start_bunzip's magic and level)
//   dd_level_scan  bz_max_level of a multistream input: every byte-aligned "BZh<d>" from input byte 4 on whose 10 bytes lie inside
//                  the input and are followed by a block or end-of-stream magic -> atomicMax of d into the input's level
//   dd_eos_bytes   per end-of-stream candidate, EOS_REC bytes from the stored stream CRC on (bz_walk reads the CRC and the
//                  restart header behind it), zeros at and past the candidate's input end
#include "decode_dev.h"
#include <algorithm>

namespace cjs {

__global__ __launch_bounds__(256) void dd_headers(const uint8_t* __restrict__ in, const uint64_t* __restrict__ off, uint32_t count, DevHdr* __restrict__ hdr) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= count) return;
  const uint64_t a = off[k], m = off[k + 1] - a;
  DevHdr h;
#pragma unroll
  for (int i = 0; i < 4; i++) h.h[i] = (uint64_t)i < m ? in[a + i] : (uint8_t)0;
  h.level = 0;
  hdr[k] = h;
}

// bytes [b0, b1) of `in` (inside [off[0], off[count])) are tested; every read stays inside the input that holds the byte
__global__ __launch_bounds__(256) void dd_level_scan(const uint8_t* __restrict__ in, const uint64_t* __restrict__ off, uint32_t count, uint64_t b0, uint64_t b1,
                                                     DevHdr* __restrict__ hdr) {
  const uint64_t b = b0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= b1 || in[b] != 'B') return;
  uint32_t lo = 0, hi = count;                        // off[lo] <= b < off[hi]: the input holding b (empty inputs share the next one's start)
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (off[mid] <= b) lo = mid; else hi = mid; }
  if (b < off[lo] + 4 || b + 10 > off[lo + 1]) return;
  if (in[b + 1] != 'Z' || in[b + 2] != 'h' || in[b + 3] < '1' || in[b + 3] > '9') return;
  uint64_t m = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) m = (m << 8) | in[b + 4 + i];
  if (m == MAGIC_BLOCK || m == MAGIC_END) atomicMax(&hdr[lo].level, (uint32_t)(in[b + 3] - '0'));
}

// tab: (first byte, input end) per record, in `in`'s absolute bytes
__global__ __launch_bounds__(256) void dd_eos_bytes(const uint8_t* __restrict__ in, const uint64_t* __restrict__ tab, uint32_t n, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t at = tab[2 * i], end = tab[2 * i + 1];
#pragma unroll
  for (int j = 0; j < EOS_REC; j++) out[(size_t)i * EOS_REC + j] = at + j < end ? in[at + j] : (uint8_t)0;
}

// one workgroup per piece: every input of a batch group and its pieces at once (20,000 tiny inputs are one launch); reads stay
// inside the piece's bytes of its input, stores are whole aligned words inside the input's 4-byte-rounded place
__global__ __launch_bounds__(256) void dd_gather(const uint8_t* __restrict__ in, const GatherPiece* __restrict__ pc, uint8_t* __restrict__ dst) {
  const GatherPiece p = pc[blockIdx.x];
  const uint8_t* __restrict__ s = in + p.src;
  uint32_t* __restrict__ d = reinterpret_cast<uint32_t*>(dst + p.dst);
  const uint32_t words = (p.len + 3) >> 2;
  for (uint32_t w = threadIdx.x; w < words; w += 256) {
    const uint32_t j = 4 * w;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) if (j + i < p.len) v |= (uint32_t)s[j + i] << (8 * i);
    d[w] = v;
  }
}

void launch_dev_gather(hipStream_t s, const uint8_t* d_in, const GatherPiece* d_pc, uint32_t npieces, uint8_t* dst) {
  if (npieces) hipLaunchKernelGGL(dd_gather, dim3(npieces), dim3(256), 0, s, d_in, d_pc, dst);
}
void launch_dev_headers(hipStream_t s, const uint8_t* d_in, const uint64_t* d_off, uint32_t count, bool multistream, uint64_t b0, uint64_t b1, DevHdr* d_hdr) {
  hipLaunchKernelGGL(dd_headers, dim3((count + 255) / 256), dim3(256), 0, s, d_in, d_off, count, d_hdr);
  if (!multistream) return;
  for (uint64_t a = b0; a < b1; a += 1ull << 31) {                   // (slabs: a grid may not exceed 2^32 threads)
    const uint64_t e = std::min<uint64_t>(b1, a + (1ull << 31));
    hipLaunchKernelGGL(dd_level_scan, dim3((unsigned)((e - a + 255) / 256)), dim3(256), 0, s, d_in, d_off, count, a, e, d_hdr);
  }
}
void launch_dev_eos_bytes(hipStream_t s, const uint8_t* d_in, const uint64_t* d_tab, uint32_t n, uint8_t* d_out) {
  hipLaunchKernelGGL(dd_eos_bytes, dim3((n + 255) / 256), dim3(256), 0, s, d_in, d_tab, n, d_out);
}

}  // namespace cjs
