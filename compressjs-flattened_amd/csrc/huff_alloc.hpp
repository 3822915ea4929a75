// huff_alloc.hpp — one wave builds one length-limited Huffman table (StaticHuffman ctor Bzip2:1866-1894 + HuffmanAllocator
// :1085-1301): rank sort by the wave, pass 1 of the in-place allocator on lane 0 with the node array in LDS, passes 2 and 3 by
// the whole wave.  The allocator's rules are huff_rules.h; here is their wave form.  Included by huff_tables.hip only: the
// phase clock g_bt_clk is read back there.
#pragma once
#include "cjs_internal.h"
#include "prims.hpp"
#include "huff_rules.h"

namespace cjs {

__device__ uint64_t g_bt_clk[8];          // table-build phase clock of (block 0, wave 0), CJS_DEBUG
#define BT_MARK(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_bt_clk[i] = wall_clock64(); } while (0)

// Passes 2 and 3 by the whole wave.  ha_first() is a search for the first node whose parent lies above `limit`, and parents
// are non-decreasing along the array, so it is ONE ballot per 64 nodes over a register copy of the parent pointers instead of
// ~10 dependent LDS reads of one lane (~60 ns each); the fills of pass 3 are one masked store.  Only nodes at or below `limit`
// are searched: pass 3 never overwrites those (it fills from the top down to `next` >= `first` > limit), and the node at `limit`
// always qualifies (its parent was created after it), which is the case in which the serial rule stays inside [lo, limit] too.
// Should it not qualify, the serial rule is applied as it stands.  All control values are wave-uniform.
__device__ __forceinline__ int haw_first(const int (&pm)[5], const int* a, int len, int limit, int lo) {
  const int lane = lane_id();
#pragma unroll
  for (int t = 0; t < 5; t++) {
    if (64 * t <= limit) {
      const int idx = lane + 64 * t;
      const uint64_t m = __ballot(idx >= lo && idx <= limit && pm[t] > limit);
      if (m) return 64 * t + (int)__builtin_ctzll(m);
    }
  }
  return ha_first(a, len, limit, lo);
}
__device__ __forceinline__ void haw_fill(int* a, int lo, int hi, int x) {          // a[lo..hi] = x
  const int lane = lane_id();
#pragma unroll
  for (int t = 0; t < 5; t++) { const int idx = lane + 64 * t; if (idx >= lo && idx <= hi) a[idx] = x; }
}
__device__ __forceinline__ void ha_passes23_wave(int* a, int len, int maxlen) {
  const int lane = lane_id();
  int pm[5];
#pragma unroll
  for (int t = 0; t < 5; t++) { const int idx = lane + 64 * t; pm[t] = idx < len ? ha_mod(a[idx], len) : 0; }
  const int root0 = __builtin_amdgcn_readfirstlane(pm[0]);                         // ha_mod(a[0], len)
  BT_MARK(2);
  ha_passes23(len, maxlen, root0,
              [&](int limit, int lo) { return haw_first(pm, a, len, limit, lo); },
              [&](int lo, int hi, int x) { haw_fill(a, lo, hi, x); },
              [&](int i) {                                                         // (the array as it stands: fills included, as in the serial form)
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xc07f);
                return __builtin_amdgcn_readfirstlane(a[i]);
              },
              [&]() { BT_MARK(3); });
}

// One wave builds one table: freq[0..n) -> lens[0..n).  key/work are per-table LDS scratch (n entries).
// (forced inline: as a call the LDS pointers are generic and every access a flat_load / flat_store.  Pass 1 of the allocator
// stays on one lane: a variant with the node array in the wave's registers -- v_readlane reads, scalar control flow -- ran its
// ~600 dependent steps no faster)
__device__ __forceinline__ void build_table_wave(const uint32_t* freq, uint8_t* lens, uint32_t* key, int* work, int n) {
  const int lane = lane_id();
  BT_MARK(0);
  for (int i = lane; i < n; i += 64) key[i] = rank_key(freq[i], (uint32_t)i);     // Bzip2:1881-1883
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  int rk[5] = {0, 0, 0, 0, 0};
  uint32_t ki[5];
#pragma unroll
  for (int t = 0; t < 5; t++) { const int i = lane + 64 * t; ki[t] = i < n ? key[i] : 0u; }
#pragma unroll 6
  for (int k = 0; k < n; k++) {                 // one broadcast read per key, compared with all five of the lane's keys
    const uint32_t kv = key[k];
#pragma unroll
    for (int t = 0; t < 5; t++) rk[t] += kv < ki[t];
  }
  __builtin_amdgcn_wave_barrier();
  for (int t = 0, i = lane; t < 5; t++, i += 64) if (i < n) work[rk[t]] = (int)(freq[i]);   // sortedFreq
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  BT_MARK(1);
  int go = 0;
  if (lane == 0) go = ha_pass1(work, n) ? 1 : 0;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  if (__builtin_amdgcn_readfirstlane(go)) ha_passes23_wave(work, __builtin_amdgcn_readfirstlane(n), MAX_BITS);
  BT_MARK(5);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  for (int t = 0, i = lane; t < 5; t++, i += 64) if (i < n) lens[i] = (uint8_t)work[rk[t]];
  BT_MARK(6);
}

}  // namespace cjs
