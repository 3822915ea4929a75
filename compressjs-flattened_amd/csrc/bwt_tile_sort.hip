// bwt_tile_sort.hip — the tile sorters of the suffix sort's rounds >= 2 (the map: bwt.hip).
// Most unresolved groups are tiny, and the array is already ordered by group, so only the order INSIDE each group is missing:
// every group of <= 1024 suffixes is sorted in LDS by the window that owns it.  The window rule -- which window owns a group,
// which one fetches a slot's rank -- is bwt_rules.h; both sorters go through ts_window below for it and keep only their own
// sort.  bwt_tile_sort: windows whose owned groups all have <= 64 members rank every member by counting inside its group;
// other windows bitonic-sort on (head slot, rank key, suffix): slots that are not owned carry their own slot number and stay
// where they are.  Groups of > 1024 suffixes keep their defer flag (preset to 1 by the host): bwt_defer.hip.
#include "bwt_dev.hpp"

namespace cjs {

// Fused rank gather: the tile sorters of rounds >= 2 make the round's keys themselves -- the groups from the head bytes that
// the regroup before left (ghead[]: one byte per slot, 1 = starts a group; a group ordinal is never needed, only where a group
// starts), rank of suffix val + h out of R -- instead of reading back a key array that bwt_gather_keys wrote: the
// random rank fetches (bound by the number of 64-byte transactions) then overlap the VALU-bound sorting of the other
// workgroups of the CU, and 16 B per suffix of key traffic are gone.  Every slot has ONE window that fetches its rank
// (ts_fetches): the window that owns its group stores the flag bytes of the group's slots at their sorted places, no keys; the
// window whose nominal range holds a slot that nobody owns stores the key as gathered, for the deferral kernels.
// slot of step s of a thread: 64 consecutive slots per wave instruction in both layouts (word of a slot = slot >> 6)
template <bool WMAP> __device__ __forceinline__ uint32_t ts_slot(int s, int tid) {
  return WMAP ? (uint32_t)(tid >> 6) * 1024u + (uint32_t)s * 64u + (uint32_t)(tid & 63) : (uint32_t)s * 256u + (uint32_t)tid;
}
// Loads of the fused form (all issued before the first use): suffixes and sorted positions of the window in the thread's slot
// layout; the head bytes of slots [16 * tid, +16) of the window as a 16-bit mask (the same slots in both layouts: the mask words
// do not depend on WMAP); and where the last head among this thread's four of the TS_MAXGRP slots in front of the window lies.
template <bool WMAP, typename TG>
__device__ __forceinline__ uint32_t ts_fused_load(const TG& tg, const uint32_t* __restrict__ val, uint64_t wb, uint32_t L,
                                                  uint32_t& heads16, uint32_t (&pv)[16], uint32_t (&pp)[16]) {
  const int tid = threadIdx.x;
  uint32_t hvalid;
  const uint4 hv = hf_load16(tg.ghead, wb, L, tid, hvalid);      // (window bases are multiples of 16)
#pragma unroll
  for (int s = 0; s < 16; s++) { const uint32_t x = ts_slot<WMAP>(s, tid); pv[s] = val[wb + (x < L ? x : L - 1u)]; }
#pragma unroll
  for (int s = 0; s < 16; s++) { const uint32_t x = ts_slot<WMAP>(s, tid); pp[s] = tg.pos[wb + (x < L ? x : L - 1u)]; }
  uint32_t li = 0;
  if (wb) li = ts_li4((uint32_t)tid, hf_bits4(*reinterpret_cast<const uint32_t*>(tg.ghead + wb - TS_MAXGRP + (uint32_t)tid * 4u), 0));      // wb is a multiple of TS_NOM >= TS_MAXGRP
  heads16 = hf_bits16(hv, 0) & hvalid;
  return li;
}
// rank keys of the slots in `need` (bit s = step s): R[suffix + h] + 1 of the suffix's block, 0 past the end (sentinel form)
template <typename TG>
__device__ __forceinline__ void ts_fused_gather(const TG& tg, uint32_t need, const uint32_t (&pv)[16], uint32_t (&pp)[16], uint32_t (&rk20)[16]) {
  uint32_t past = 0, blk = pp[0] / tg.g.stride;      // the thread's slots ascend with s in both layouts, and pos[] with the slot
#pragma unroll
  for (int s = 0; s < 16; s++) {
    blk = blk_step(pp[s], tg.g.stride, blk);
    const uint32_t n = blk_len(tg.g, blk);
    uint32_t j = pk_pos(pv[s]) + tg.h;      // (the top byte of val[] may carry the byte in front of the suffix)
    if (tg.cyclic) { if (j >= n) j %= n; }
    else if (j >= n) { j = 0; past |= 1u << s; }
    pp[s] = blk * tg.g.stride + j;               // (positions are 32 bits wide: bwt_run refuses more)
  }
#pragma unroll
  for (int s = 0; s < 16; s++) rk20[s] = tg.R[((need >> s) & 1u) ? pp[s] : pp[0]];
#pragma unroll
  for (int s = 0; s < 16; s++) rk20[s] = ((past >> s) & 1u) ? 0u : rk20[s] + 1u;
}

// The window prologue of both tile sorters, from the loads to the store of the keys that are not sorted here: finds the heads
// among the window's L slots, classifies every slot by the window rule (bwt_rules.h), clears the defer flags of the owned
// ones, fetches the rank keys of the slots that this window answers for and stores, for those it does not own, the key as
// gathered.  each(s, x, hx, nx, owned, medium) runs once per step s, for all threads together: slot x, its group [hx, nx) in
// window slots (nx closed by ts_close) and how this window holds it.  Leaves pv = the suffixes and rk20 = the rank keys of the
// fetched slots; returns the mask of the owned steps.
template <bool WMAP, typename TG, typename Each>
__device__ __forceinline__ uint32_t ts_window(uint64_t* __restrict__ key, const uint32_t* __restrict__ val, uint8_t* __restrict__ dflag, const TG& tg,
                                              uint64_t wb, uint32_t L, bool at_end, uint32_t (&pv)[16], uint32_t (&rk20)[16], Each&& each) {
  __shared__ uint64_t hm[64];                    // head mask of the window
  __shared__ int32_t wlast[64], wnext[64];       // last head before word / first head after word (window slot, TS_NO_HEAD / TS_NO_NEXT = none)
  __shared__ uint32_t lired[4];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  uint32_t pp[16], heads16;
  // every global load of the window (head bytes, suffixes, positions) is issued before the first LDS store: written as one loop
  // the compiler waits for each load in turn, sixteen memory round trips instead of one
  const uint32_t li = wave_max(ts_fused_load<WMAP>(tg, val, wb, L, heads16, pv, pp));
  if (lane == 0) lired[w] = li;
  reinterpret_cast<uint16_t*>(hm)[tid] = (uint16_t)heads16;      // the head mask is the head bytes themselves: 16 bits per thread, laid over the 64 words
  __syncthreads();
  if (w == 0) {      // per mask word: last head strictly before the word, first head strictly after it
    const uint64_t m = hm[lane];
    uint32_t incl;
    wlast[lane] = (int)last_head_before_word(m, lane, incl) - 1;
    // suffix min of the words' first heads: max-scan on the reversed lane order of the negated value
    const int rv = __shfl(-word_first(m, lane), 63 - lane, 64);
    const int ir = wave_incl_max(rv);
    int er = __shfl_up(ir, 1, 64); if (lane == 0) er = -TS_NO_NEXT;
    wnext[lane] = -__shfl(er, 63 - lane, 64);
  }
  __syncthreads();
  const uint32_t a01 = lired[0] > lired[1] ? lired[0] : lired[1], a23 = lired[2] > lired[3] ? lired[2] : lired[3];
  const uint32_t prev_end = ts_prev_end(wb, L, at_end, a01 > a23 ? a01 : a23, hm[0], wnext[0]);
  uint32_t ownm = 0, needm = 0, headm = 0;
#pragma unroll
  for (int s = 0; s < 16; s++) {
    const uint32_t x = ts_slot<WMAP>(s, tid);
    const int wi = (int)(x >> 6);
    const uint64_t m = hm[wi];
    headm |= (uint32_t)((m >> lane) & 1ull) << s;      // (lane = x & 63 in both layouts)
    const int hx = ts_head_of(m, wi, lane, wlast[wi]), nx = ts_next_of(m, wi, lane, wnext[wi]);
    const TsOwn own = ts_classify(hx, nx, L, at_end);
    const bool owned = x < L && own.owned;
    if (owned && dflag) dflag[wb + x] = 0;
    ownm |= owned ? 1u << s : 0u;
    needm |= ts_fetches(x < L, x, prev_end, owned) ? 1u << s : 0u;
    each(s, x, hx, ts_close(nx, L, at_end), owned, owned && own.medium);
  }
  ts_fused_gather(tg, needm, pv, pp, rk20);
#pragma unroll
  for (int s = 0; s < 16; s++)
    if (((needm >> s) & 1u) && !((ownm >> s) & 1u)) key[wb + ts_slot<WMAP>(s, tid)] = round_key((headm >> s) & 1u, rk20[s]);      // not sorted here: head bit | rank key, for the deferral
  return ownm;
}

__device__ __forceinline__ void ts_ce(uint64_t& a, uint64_t& b, bool up) {
  const bool sw = (a > b) == up;
  const uint64_t x = sw ? b : a, y = sw ? a : b;
  a = x; b = y;
}
template <typename TG>
__global__ __launch_bounds__(256) void bwt_tile_sort(uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint8_t* __restrict__ hflag, uint32_t A,
                                                     uint8_t* __restrict__ dflag, TG tg, uint32_t Tt) {
  __shared__ uint64_t sk[TS_WIN];                // the sort: 32-bit counting words, then the compacted members of the larger groups
  __shared__ uint64_t mm[64];                   // mask of the owned slots in groups of > TS_TINY members
  __shared__ uint32_t mpre[65];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint32_t win = xcd_tile(blockIdx.x, Tt);            // windows of one block on one XCD: its ranks stay in that L2
  if (win >= Tt) return;
  const uint64_t wb = ts_win_base(win);
  const uint32_t L = ts_win_len(wb, A);
  uint64_t r[16];
  uint32_t pv[16];
  int any_medium = 0;
  uint32_t hx16[16];          // head slot (low 16 bits) | group size (high 16 bits) of owned slots, 0xFFFFFFFF otherwise
  uint32_t rk20[16];
  ts_window<false>(key, val, dflag, tg, wb, L, wb + L == A, pv, rk20,
                   [&](int it, uint32_t x, int hx, int nx, bool owned, bool medium) {
    hx16[it] = owned ? ((uint32_t)hx | ((uint32_t)(nx - hx) << 16)) : 0xFFFFFFFFu;
    const uint64_t mb = __ballot(medium);
    if (lane == 0) mm[x >> 6] = mb;
    any_medium |= medium ? 1 : 0;
  });
#pragma unroll
  for (int it = 0; it < 16; it++) r[it] = hx16[it] != 0xFFFFFFFFu ? ts64_owned(hx16[it] & 0xFFFFu, rk20[it], pv[it]) : ts64_other((uint32_t)it * 256u + tid);
  // groups of <= TS_TINY members: every member counts the smaller members of its group.  Inside a group only the
  // 20-bit rank key matters (equal keys stay one group, any order): 32-bit words (key << 12 | slot) are compared
  uint32_t* sk32 = reinterpret_cast<uint32_t*>(sk);
#pragma unroll
  for (int it = 0; it < 16; it++) { const uint32_t x = (uint32_t)it * 256u + tid; sk32[x] = ts64_count_word(r[it], x); }
  any_medium = __syncthreads_or(any_medium);
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const bool own = hx16[it] != 0xFFFFFFFFu && (hx16[it] >> 16) <= TS_TINY;
    const uint32_t hx = own ? (hx16[it] & 0xFFFFu) : 0u, g = own ? (hx16[it] >> 16) : 0u;
    const uint32_t gmax = wave_max(g);
    if (gmax == 0) continue;
    const uint64_t mine = r[it];
    const uint32_t mine32 = ts64_count_word(mine, (uint32_t)it * 256u + tid);
    uint32_t rank = 0, same = 0;        // same: members with my rank key that sort in front of me (none: I start a new group)
    for (uint32_t d = 0; d < gmax; d++) {
      const uint32_t o = sk32[hx + d];
      const bool lt = d < g && o < mine32;
      rank += lt ? 1u : 0u;
      same += (lt && (o >> 12) == (mine32 >> 12)) ? 1u : 0u;
    }
    if (own) {
      hflag[wb + hx + rank] = hf_byte(!same, !rank);
      val[wb + hx + rank] = (uint32_t)mine;
    }
  }
  if (!any_medium) return;
  // larger groups: compact their members (the order of slots is kept), bitonic-sort the compacted array on
  // (head slot, rank key, suffix), and hand the c-th element to the c-th compacted slot
  if (w == 0) {
    const uint32_t pc = (uint32_t)__builtin_popcountll(mm[lane]);
    const uint32_t inc = wave_incl_sum(pc);
    mpre[lane] = inc - pc;
    if (lane == 63) mpre[64] = inc;
  }
  __syncthreads();            // also: all counting reads of sk are done
  const uint32_t Mt = mpre[64];
  uint32_t P = 2;
  while (P < Mt) P <<= 1;
  uint32_t cix[16];
#pragma unroll
  for (int it = 0; it < 16; it++) {
    const int wi = it * 4 + w;
    const uint64_t mb = mm[wi];
    const bool medium = (mb >> lane) & 1ull;
    cix[it] = medium ? mpre[wi] + (uint32_t)__builtin_popcountll(mb & ((1ull << lane) - 1ull)) : 0xFFFFFFFFu;
    if (medium) sk[cix[it]] = r[it];
  }
  for (uint32_t c = Mt + tid; c < P; c += 256) sk[c] = ~0ull;
  __syncthreads();
  for (uint32_t kk = 2; kk <= P; kk <<= 1) {
    uint32_t j = kk >> 1;
    if (__builtin_popcount(kk - 1) & 1) {      // odd number of steps in this merge phase: one single step first
      for (uint32_t t = tid; t < (P >> 1); t += 256) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const uint32_t l = i | j;
        const uint64_t a = sk[i], b = sk[l];
        const bool up = (i & kk) == 0;
        if ((a > b) == up) { sk[i] = b; sk[l] = a; }
      }
      __syncthreads();
      j >>= 1;
    }
    for (; j > 0; j >>= 2) {                   // steps j and j/2 in one LDS round trip, 4 elements per thread
      const uint32_t hj = j >> 1;
      for (uint32_t t = tid; t < (P >> 2); t += 256) {
        const uint32_t i0 = ((t & ~(hj - 1)) << 2) | (t & (hj - 1));
        const bool up = (i0 & kk) == 0;
        uint64_t e0 = sk[i0], e1 = sk[i0 | hj], e2 = sk[i0 | j], e3 = sk[i0 | j | hj];
        ts_ce(e0, e2, up); ts_ce(e1, e3, up); ts_ce(e0, e1, up); ts_ce(e2, e3, up);
        sk[i0] = e0; sk[i0 | hj] = e1; sk[i0 | j] = e2; sk[i0 | j | hj] = e3;
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int it = 0; it < 16; it++) {
    if (cix[it] != 0xFFFFFFFFu) {
      const uint32_t x = (uint32_t)it * 256u + tid;
      const uint32_t c = cix[it];
      const uint64_t e = sk[c], pe = c ? sk[c - 1] : ~e;          // (head slot, rank key) of the sorted predecessor
      hflag[wb + x] = hf_byte((e >> 32) != (pe >> 32), (e >> 52) != (pe >> 52));
      val[wb + x] = (uint32_t)e;
    }
  }
}
// LDS radix version of the tile sorter.  Every slot of the window gets a 32-bit composite (head slot of its group << 20 |
// 20-bit rank key); slots that are not owned carry (own slot << 20).  A stable LSD radix sort of the whole window on that
// composite (4 passes of 8 bits, wave64 match-any ranking, one LDS staging array) is then a permutation INSIDE every owned
// group: exactly h slots carry a composite below (h << 20), so the members of the group headed at h land on [h, h + size).
// The cost does not depend on the group sizes (the counting / bitonic version above degrades with them).
template <typename TG>
__global__ __launch_bounds__(256) void bwt_tile_sort_radix(uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint8_t* __restrict__ hflag, uint32_t A,
                                                           uint8_t* __restrict__ dflag, TG tg, uint32_t Tt) {
  __shared__ uint64_t se[TS_WIN];                // (composite << 32) | suffix: staging of a pass
  __shared__ uint32_t wcnt[4][256];
  __shared__ uint32_t sm[4];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint32_t win = xcd_tile(blockIdx.x, Tt);            // windows of one block on one XCD: its ranks stay in that L2
  if (win >= Tt) return;
  const uint64_t wb = ts_win_base(win);
  const uint32_t L = ts_win_len(wb, A);
  // slot of (wave w, step s, lane): w * 1024 + s * 64 + lane -- array order = (w, s, lane) order, which the stable ranking needs
  uint32_t rk20[16], pv[16], comp[16];
  const uint32_t ownm = ts_window<true>(key, val, dflag, tg, wb, L, wb + L == A, pv, rk20,
                                        [&](int s, uint32_t, int hx, int, bool, bool) { comp[s] = (uint32_t)hx; });
#pragma unroll
  for (int s = 0; s < 16; s++) {
    const bool owned = (ownm >> s) & 1u;
    comp[s] = owned ? ts32_owned(comp[s], rk20[s]) : ts32_other(ts_slot<true>(s, tid));
    if (!owned) pv[s] = 0u;
  }
  if (!__syncthreads_or((int)ownm)) return;
#pragma unroll 1
  for (int shift = 0; shift < 32; shift += 8) {
    for (int i = tid; i < 1024; i += 256) (&wcnt[0][0])[i] = 0;
    __syncthreads();
    uint32_t rk[16];
#pragma unroll
    for (int s = 0; s < 16; s++) rk[s] = rank_step((comp[s] >> shift) & 255u, wcnt[w]);
    __syncthreads();
    {
      const uint32_t c0 = wcnt[0][tid], c1 = wcnt[1][tid], c2 = wcnt[2][tid], c3 = wcnt[3][tid];
      uint32_t total;
      const uint32_t ex = block_excl_sum<256>(c0 + c1 + c2 + c3, sm, total);
      wcnt[0][tid] = ex; wcnt[1][tid] = ex + c0; wcnt[2][tid] = ex + c0 + c1; wcnt[3][tid] = ex + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const uint32_t d = (comp[s] >> shift) & 255u;
      se[wcnt[w][d] + rk[s]] = ((uint64_t)comp[s] << 32) | pv[s];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const uint64_t e = se[(uint32_t)w * 1024u + (uint32_t)s * 64u + lane];
      comp[s] = (uint32_t)(e >> 32); pv[s] = (uint32_t)e;
    }
    __syncthreads();
  }
#pragma unroll
  for (int s = 0; s < 16; s++) {
    if ((ownm >> s) & 1u) {
      const uint32_t x = (uint32_t)w * 1024u + (uint32_t)s * 64u + lane;
      const uint32_t pc = x ? (uint32_t)(se[x - 1] >> 32) : ~comp[s];      // composite of the sorted predecessor (se[] still holds the last pass)
      hflag[wb + x] = hf_of_sorted(comp[s], pc);
      val[wb + x] = pv[s];
    }
  }
}

template <typename TG>
void launch_tile_sort(hipStream_t s, uint64_t* key, uint32_t* val, uint8_t* hflag, uint32_t A, uint8_t* dflag, uint32_t ngroups, const TG& tg) {
  const uint32_t Tt = ts_windows(A);
  if (radix_tile_sorter(A, ngroups)) hipLaunchKernelGGL(bwt_tile_sort_radix<TG>, dim3(xcd_grid(Tt)), dim3(256), 0, s, key, val, hflag, A, dflag, tg, Tt);
  else hipLaunchKernelGGL(bwt_tile_sort<TG>, dim3(xcd_grid(Tt)), dim3(256), 0, s, key, val, hflag, A, dflag, tg, Tt);
}
template void launch_tile_sort<TsGatherT<Geom>>(hipStream_t, uint64_t*, uint32_t*, uint8_t*, uint32_t, uint8_t*, uint32_t, const TsGatherT<Geom>&);
template void launch_tile_sort<TsGatherT<VarGeom>>(hipStream_t, uint64_t*, uint32_t*, uint8_t*, uint32_t, uint8_t*, uint32_t, const TsGatherT<VarGeom>&);

}  // namespace cjs
