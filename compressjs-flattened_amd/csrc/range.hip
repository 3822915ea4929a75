// range.hip -- the kernels of the indexed range reads (cjs_bzip2_read_ranges[_device], decode.hip):
//   rg_slices       the slice gather: every piece (source address, destination address, length) of a pass in one launch per slab.
//                   It moves the ranges' bytes out of a pass's expanded blocks (to the packed device buffer of the host form, or
//                   straight into the caller's d_out), and it is the device form's upload: the byte runs of the touched blocks,
//                   out of the caller's d_in into the pass's upload buffer.
//   rg_cand_magic   the 48-bit block magic at every candidate the index names (there is no magic scan on this path)
#include "decode_dev.h"
#include <algorithm>

namespace cjs {

// The aligned 16 bytes at address p of a source that is bytes [lo, hi): a vector load when they all belong to it; at the two ends
// of a source the bytes that do, one by one, zeros for the others (nothing outside the source is read).
__device__ __forceinline__ uint4 rg_ld16(uint64_t p, uint64_t lo, uint64_t hi) {
  if (p >= lo && p + 16 <= hi) return *reinterpret_cast<const uint4*>(p);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 16; i++) if (p + i >= lo && p + i < hi) w[i >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(p + i) << (8 * (i & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// The interior of a piece: nvec 16-byte vectors, the destination da aligned, the source sa = 16 * q + 4 * K + m behind an aligned
// address.  Lane i stores vector i (consecutive lanes, consecutive 16 bytes) from the two aligned source vectors it straddles:
// dword j of the result is dwords K + j and K + j + 1 of the eight, funnelled by m bytes.  K and m are the same for every vector
// of the piece, so the choice is made once per workgroup.
template <int K>
__device__ __forceinline__ void rg_interior(uint64_t sa, uint64_t da, uint64_t nvec, uint32_t m, uint64_t lo, uint64_t hi) {
  for (uint64_t v = threadIdx.x; v < nvec; v += 256) {
    const uint64_t base = (sa + 16 * v) & ~15ull;
    const uint4 a = rg_ld16(base, lo, hi);
    const uint4 b = (K || m) ? rg_ld16(base + 16, lo, hi) : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(w[K + 1], w[K], m);
    o.y = __builtin_amdgcn_alignbyte(w[K + 2], w[K + 1], m);
    o.z = __builtin_amdgcn_alignbyte(w[K + 3], w[K + 2], m);
    o.w = __builtin_amdgcn_alignbyte(w[K + 4], w[K + 3], m);
    *reinterpret_cast<uint4*>(da + 16 * v) = o;
  }
}

// One workgroup per piece (at most SLICE_TASK bytes: the host cuts longer ones).  Source and destination are at any byte
// alignment, also relative to each other.  Bytes in front of the destination's first 16-byte boundary and behind its last are
// byte stores; everything between is aligned 16-byte stores.  Writes stay inside [dst, dst + len), reads inside [src, src + len).
__global__ __launch_bounds__(256) void rg_slices(const Slice* __restrict__ sl, uint32_t s0) {
  const Slice t = sl[s0 + blockIdx.x];
  const uint64_t s = t.src, d = t.dst, len = t.len;
  const uint32_t head = (uint32_t)min(len, (0ull - d) & 15ull);
  const uint64_t nvec = (len - head) >> 4;
  const uint32_t tail = (uint32_t)((len - head) & 15u);
  if (threadIdx.x < head) *reinterpret_cast<uint8_t*>(d + threadIdx.x) = *reinterpret_cast<const uint8_t*>(s + threadIdx.x);
  if (threadIdx.x < tail) {
    const uint64_t o = head + 16 * nvec + threadIdx.x;
    *reinterpret_cast<uint8_t*>(d + o) = *reinterpret_cast<const uint8_t*>(s + o);
  }
  if (!nvec) return;
  const uint64_t sa = s + head, da = d + head;
  const uint32_t m = (uint32_t)(sa & 3u);
  switch ((uint32_t)(sa & 15u) >> 2) {
    case 0: rg_interior<0>(sa, da, nvec, m, s, s + len); break;
    case 1: rg_interior<1>(sa, da, nvec, m, s, s + len); break;
    case 2: rg_interior<2>(sa, da, nvec, m, s, s + len); break;
    default: rg_interior<3>(sa, da, nvec, m, s, s + len); break;
  }
}

// ok[c] = the 48 bits at bits[c] of `in` (n bytes) are the block magic, wholly inside the n bytes
__global__ __launch_bounds__(256) void rg_cand_magic(const uint8_t* __restrict__ in, uint64_t n, const uint64_t* __restrict__ bits, uint32_t nc, uint32_t* __restrict__ ok) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nc) return;
  const uint64_t bit = bits[c], byte = bit >> 3;
  uint64_t w = 0;
  for (int i = 0; i < 7; i++) w = (w << 8) | (byte + i < n ? in[byte + i] : 0);      // 56 bits
  const uint64_t v = (w >> (8 - (bit & 7))) & 0xFFFFFFFFFFFFull;
  ok[c] = (bit + 48 <= n * 8 && v == MAGIC_BLOCK) ? 1u : 0u;
}

void launch_slices(hipStream_t s, const Slice* d_sl, size_t n) {
  for (size_t s0 = 0; s0 < n; s0 += SLICE_SLAB) hipLaunchKernelGGL(rg_slices, dim3((unsigned)std::min(SLICE_SLAB, n - s0)), dim3(256), 0, s, d_sl, (uint32_t)s0);
}
void launch_cand_magic(hipStream_t s, const uint8_t* d_in, uint64_t n, const uint64_t* d_bits, uint32_t nc, uint32_t* d_ok) {
  if (nc) hipLaunchKernelGGL(rg_cand_magic, dim3((nc + 255) / 256), dim3(256), 0, s, d_in, n, d_bits, nc, d_ok);
}

}  // namespace cjs
