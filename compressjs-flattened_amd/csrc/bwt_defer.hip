// bwt_defer.hip — the deferral trip of the suffix sort's rounds >= 2 (the map: bwt.hip; sort_round there drives it): the groups
// that no tile-sorter window owns keep their defer flag; they are counted, compacted, sorted by the radix passes and put back.
#include "bwt_dev.hpp"

namespace cjs {

// single workgroup: exclusive scan of n counters in place, total -> *total
__global__ __launch_bounds__(1024) void scan_u32_single(uint32_t* __restrict__ arr, uint32_t n, uint32_t* __restrict__ total, uint32_t* __restrict__ host_total) {
  __shared__ uint32_t sm[16];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    uint32_t v = i < n ? arr[i] : 0u, tot;
    const uint32_t ex = block_excl_sum<1024>(v, sm, tot);
    if (i < n) arr[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) { *total = carry; *host_total = carry; }
}
// Groups too large for the tile sorters (dflag = 1 on all their slots) are compacted, sorted by the global radix passes and
// put back.  Numbered densely among themselves (there are at most A / 1025 of them) their ordinals take ~11 bits of the sort
// key: a deferred slot starts a deferred group when its key carries the head bit (the tile sorters store head bit | rank key for
// the slots they do not own; a group is deferred whole).  Per 2048-slot tile: deferred slots -> tcount, deferred heads -> hcount.
__device__ __forceinline__ void defer_flags(uint32_t A, const uint8_t* __restrict__ dflag, const uint64_t* __restrict__ key, uint64_t a0,
                                            uint32_t& f, uint32_t& heads, uint64_t (&k8)[8]) {
  f = 0; heads = 0;
  if (a0 >= A) return;
  if (a0 + 8 <= A) {
    const uint64_t w = *(const uint64_t*)(dflag + a0);
#pragma unroll
    for (int j = 0; j < 8; j++) f |= (uint32_t)((w >> (8 * j)) & 1ull) << j;
  } else for (int j = 0; j < 8; j++) if (a0 + j < A && dflag[a0 + j]) f |= 1u << j;
  if (!f) return;
#pragma unroll
  for (int j = 0; j < 8; j++) k8[j] = a0 + j < A ? key[a0 + j] : 0ull;
#pragma unroll
  for (int j = 0; j < 8; j++) heads |= (uint32_t)(round_key_ordinal(k8[j]) & 1ull) << j;      // (slots that are not deferred hold stale keys)
  heads &= f;
}
__global__ __launch_bounds__(256) void bwt_defer_count(uint32_t A, const uint8_t* __restrict__ dflag, const uint64_t* __restrict__ key,
                                                       uint32_t* __restrict__ tcount, uint32_t* __restrict__ hcount) {
  __shared__ uint32_t sm[4];
  const uint64_t a0 = (uint64_t)blockIdx.x * TS_GT + (uint32_t)threadIdx.x * 8u;
  uint32_t f, heads; uint64_t k8[8];
  defer_flags(A, dflag, key, a0, f, heads, k8);
  const uint32_t cnt = block_sum<256>((uint32_t)__builtin_popcount(f), sm);
  const uint32_t hc = block_sum<256>((uint32_t)__builtin_popcount(heads), sm);
  if (threadIdx.x == 0) { tcount[blockIdx.x] = cnt; hcount[blockIdx.x] = hc; }
}
__global__ __launch_bounds__(256) void bwt_defer_gather(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, uint32_t A,
                                                        const uint8_t* __restrict__ dflag, const uint32_t* __restrict__ tcount, const uint32_t* __restrict__ hcount,
                                                        uint64_t* __restrict__ dk, uint32_t* __restrict__ dv, uint32_t* __restrict__ dpos) {
  __shared__ uint32_t sm[4];
  const uint64_t a0 = (uint64_t)blockIdx.x * TS_GT + (uint32_t)threadIdx.x * 8u;
  uint32_t f, heads; uint64_t k8[8];
  defer_flags(A, dflag, key, a0, f, heads, k8);
  uint32_t tot;
  uint32_t o = tcount[blockIdx.x] + block_excl_sum<256>((uint32_t)__builtin_popcount(f), sm, tot);
  uint32_t hid = hcount[blockIdx.x] + block_excl_sum<256>((uint32_t)__builtin_popcount(heads), sm, tot);      // deferred heads in front of this thread's slots
#pragma unroll
  for (int j = 0; j < 8; j++) if ((f >> j) & 1u) {
    hid += (heads >> j) & 1u;
    dk[o] = round_key(hid - 1u, round_key_rank(k8[j])); dv[o] = val[a0 + j]; dpos[o] = (uint32_t)(a0 + j); o++;
  }
}
__global__ __launch_bounds__(256) void bwt_defer_scatter(uint32_t D, const uint64_t* __restrict__ dk, const uint32_t* __restrict__ dv,
                                                         const uint32_t* __restrict__ dpos, uint8_t* __restrict__ hflag, uint32_t* __restrict__ val) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < D; j += (uint64_t)gridDim.x * 256) {
    const uint32_t a = dpos[j];          // a slot of the same group (deferred slots and sorted records are both in group order)
    const uint64_t k = dk[j], p = j ? dk[j - 1] : ~k;      // (dense ordinal << 20 | rank key) of the record and of the one in front
    hflag[a] = hf_of_sorted(k, p); val[a] = dv[j];
  }
}

void launch_defer_count(hipStream_t s, uint32_t A, const uint8_t* dflag, const uint64_t* key, uint32_t* tcount, uint32_t* hcount, uint32_t* counters, uint32_t* h_counters) {
  const uint32_t Tg = (A + TS_GT - 1) / TS_GT;
  hipLaunchKernelGGL(bwt_defer_count, dim3(Tg), dim3(256), 0, s, A, dflag, key, tcount, hcount);
  hipLaunchKernelGGL(scan_u32_single, dim3(1), dim3(1024), 0, s, hcount, Tg, counters + CN_DEFERRED_GROUPS, h_counters + CN_DEFERRED_GROUPS);
  hipLaunchKernelGGL(scan_u32_single, dim3(1), dim3(1024), 0, s, tcount, Tg, counters + CN_DEFERRED, h_counters + CN_DEFERRED);
}
int sort_deferred(hipStream_t s, BwtWork& w, const Round& r, uint32_t D, uint32_t ndg, const uint32_t* tcount, const uint32_t* hcount, LaunchTimes* lt) {
  const int c = r.c;
  uint64_t* dk0 = w.key[1 - c]; uint64_t* dk1 = dk0 + w.cap / 2;
  uint32_t* dv0 = w.val[1 - c]; uint32_t* dv1 = dv0 + w.cap / 2;
  uint32_t* dpos = w.pos[1 - r.pc];
  hipLaunchKernelGGL(bwt_defer_gather, dim3((r.A + TS_GT - 1) / TS_GT), dim3(256), 0, s, w.key[c], w.val[c], r.A, w.dflag, tcount, hcount, dk0, dv0, dpos);
  int cur = 0;
  // (whole digits are sorted: the rest of the last one is zero, bwt_defer_gather's round_key(hid - 1, rank) has nothing above the ordinal)
  CJS_TRY((radix_passes<uint64_t>(s, w.rs, dk0, dv0, dk1, dv1, cur, D, 0, round_key_bits(ndg), lt)));      // dense ordinals 0 .. ndg-1 above the 20-bit rank key
  hipLaunchKernelGGL(bwt_defer_scatter, dim3((D + 255) / 256 < 8192u ? (D + 255) / 256 : 8192u), dim3(256), 0, s, D, cur ? dk1 : dk0, cur ? dv1 : dv0, dpos,
                     w.hflag, w.val[c]);
  return 0;
}

}  // namespace cjs
