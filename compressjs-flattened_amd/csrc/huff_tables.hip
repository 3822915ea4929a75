// huff_tables.hip — bzip2 entropy stage on the GPU, the tables: multi-table canonical Huffman construction (the reference's own
// heuristic, bit-exact) and the bit accounting of every block.
//
// Replaces J/Bzip2_joined_.js: StaticHuffman ctor :1866-1894 + HuffmanAllocator :1085-1301 (huff_alloc.hpp),
// assignSelectors :1989-2004, optimizeHuffmanGroups :2005-2054, table count :2150-2163, selector MTF :2167-2182,
// StaticHuffman.computeCanonical :1896-1916.  The rules shared with the packer (huff_pack.hip) are huff_rules.h.
// One workgroup per block: the work is tiny (<= 18 k groups of 50 symbols, <= 6 tables of <= 258
// symbols) but its logic is serial, so tables are built one per wave (rank sort by the wave,
// in-place length-limited allocator on lane 0 with the node array in LDS) and everything that is
// per-group or per-symbol is data-parallel across the 1024 lanes.
#include "cjs_internal.h"
#include "prims.hpp"
#include "huff.h"
#include "huff_alloc.hpp"

namespace cjs {

// phase clock of workgroup 0 (CJS_DEBUG only): 100 MHz ticks at the marks of huff_block
__device__ uint64_t g_huff_clk[32];
#define HB_MARK(i) do { if (dbg && blockIdx.x == 0 && threadIdx.x == 0) g_huff_clk[i] = wall_clock64(); } while (0)

struct HuffShared {
  uint32_t freq[MAXTAB][FREQ_W];
  uint32_t key[MAXTAB][FREQ_W];
  int work[MAXTAB][FREQ_W];
  uint8_t lens[MAXTAB][WL_W];
  uint32_t chist[1024];
  uint64_t packed[FREQ_W];
  uint32_t counts[8];
  uint32_t misc[8];
  uint32_t sm[16];
};

// assignSelectors (Bzip2:1989-2004).  Cost of a 50-symbol group under all tables at once: the six code
// lengths of a symbol are packed as 10-bit fields of one u64 (50 * 20 < 1024, fields cannot overflow), so the
// inner loop is one LDS read + one 64-bit add per symbol.  Symbols are staged through LDS with coalesced
// loads (512 groups = 51,200 bytes per step); lane g then reads its 25 dwords at a 25-dword stride (no bank aliasing).
__device__ void assign_selectors(HuffShared& S, uint32_t* __restrict__ stage /* AS_GROUPS*25 dwords */, const uint16_t* __restrict__ A,
                                 uint32_t npos, uint32_t nsel, int ng, uint8_t* __restrict__ sel, uint16_t* __restrict__ bcost,
                                 uint32_t g_lo = 0, uint32_t g_hi = 0xFFFFFFFFu /* groups [g_lo, g_hi): a multiple of AS_GROUPS each */) {
  if (g_hi < nsel) nsel = g_hi;
  for (int s = threadIdx.x; s < MAXSYM; s += 1024) {
    uint64_t pk = 0;
    for (int j = 0; j < ng; j++) pk |= (uint64_t)S.lens[j][s] << (10 * j);
    S.packed[s] = pk;
  }
  const uint32_t* A32 = reinterpret_cast<const uint32_t*>(A);          // A rows are 16-byte aligned (a_stride % 8 == 0)
  const uint32_t ndw = (npos + 1) / 2;
  constexpr int NPRE = (AS_GROUPS * 25 + 1023) / 1024;                 // 13 dwords per lane and step
  uint32_t pre[NPRE];                                                  // next step's symbols: loaded while this step is costed
#pragma unroll
  for (int j = 0; j < NPRE; j++) { const uint32_t i = (uint32_t)j * 1024u + threadIdx.x; pre[j] = (i < AS_GROUPS * 25 && g_lo * 25 + i < ndw) ? A32[g_lo * 25 + i] : 0u; }
  const uint32_t half = threadIdx.x & 1u, gl = threadIdx.x >> 1;       // two lanes per group: dwords [0,13) and [13,25)
  for (uint32_t g0 = g_lo; g0 < nsel; g0 += AS_GROUPS) {
    __syncthreads();                                                   // previous step's readers are done (first step: packed[] is complete)
#pragma unroll
    for (int j = 0; j < NPRE; j++) { const uint32_t i = (uint32_t)j * 1024u + threadIdx.x; if (i < AS_GROUPS * 25) stage[i] = pre[j]; }
    __syncthreads();
    {
      const uint32_t dw1 = (g0 + AS_GROUPS) * 25;
#pragma unroll
      for (int j = 0; j < NPRE; j++) {
        const uint32_t i = (uint32_t)j * 1024u + threadIdx.x;
        pre[j] = (g0 + AS_GROUPS < nsel && i < AS_GROUPS * 25 && dw1 + i < ndw) ? A32[dw1 + i] : 0u;
      }
    }
    const uint32_t g = g0 + gl;
    uint64_t acc = 0;
    if (g < nsel) {
      const uint32_t off = g * GSZ, cnt = npos - off < GSZ ? npos - off : GSZ;
      const uint32_t* my = stage + gl * 25;
      const uint32_t j0 = half ? 13u : 0u, j1 = half ? 25u : 13u;
      for (uint32_t j = j0; j < j1; j++) {
        const uint32_t w = my[j];
        if (2 * j < cnt) acc += S.packed[w & 0xFFFFu];
        if (2 * j + 1 < cnt) acc += S.packed[w >> 16];
      }
    }
    acc += __shfl_xor(acc, 1, 64);
    if (g < nsel && half == 0) {
      int best = 0; uint32_t bc = (uint32_t)(acc & 1023u);
#pragma unroll
      for (int j = 1; j < 6; j++) { const uint32_t cj = (uint32_t)((acc >> (10 * j)) & 1023u); if (j < ng && cj < bc) { best = j; bc = cj; } }
      sel[g] = (uint8_t)best; bcost[g] = (uint16_t)bc;
    }
  }
  __syncthreads();
}

// optimizeHuffmanGroups, the split of one refinement (Bzip2:2012-2042): the most used table's groups are cut at the median
// cost (stable inside the median bin, Q16); the upper half moves to the new table ng
__device__ void median_split(HuffShared& S, uint8_t* __restrict__ sel, const uint16_t* __restrict__ bcost, uint32_t nsel, int ng) {
  if (threadIdx.x < 8) S.counts[threadIdx.x] = 0;
  __syncthreads();
  {                                                     // groups per table: wave ballots (all groups aim at <= 6 counters)
    uint32_t c6[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t g0 = 0; g0 < nsel; g0 += 1024) {
      const uint32_t g = g0 + threadIdx.x;
      const uint32_t sv = g < nsel ? sel[g] : 255u;
#pragma unroll
      for (int j = 0; j < 6; j++) c6[j] += (uint32_t)__popcll(__ballot(sv == (uint32_t)j));
    }
    if (lane_id() == 0) {
#pragma unroll
      for (int j = 0; j < 6; j++) if (c6[j]) atomicAdd(&S.counts[j], c6[j]);
    }
  }
  S.chist[threadIdx.x] = 0;
  __syncthreads();
  int which = 0;
  for (int j = 1; j < ng; j++) if (S.counts[j] > S.counts[which]) which = j;      // indexOf(max): first
  const uint32_t nsp = S.counts[which], m = nsp >> 1;
  for (uint32_t g = threadIdx.x; g < nsel; g += 1024) if (sel[g] == which) atomicAdd(&S.chist[bcost[g] & 1023u], 1u);
  __syncthreads();
  {
    const uint32_t hv = S.chist[threadIdx.x];
    uint32_t tot;
    const uint32_t cum = block_excl_sum<1024>(hv, S.sm, tot);
    if (hv && cum <= m && m < cum + hv) { S.misc[0] = threadIdx.x; S.misc[1] = cum; }
    __syncthreads();
  }
  const uint32_t cstar = S.misc[0], cumstar = S.misc[1];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nsel; base += 1024) {        // stable order inside the median cost bin (Q16)
    const uint32_t g = base + threadIdx.x;
    uint32_t f = 0, mine = 0xFFFFu;
    if (g < nsel && sel[g] == which) { mine = bcost[g]; f = mine == cstar; }
    uint32_t tot;
    const uint32_t ex = block_excl_sum<1024>(f, S.sm, tot);
    if (g < nsel && mine != 0xFFFFu) {
      if (mine > cstar || (f && cumstar + carry + ex >= m)) sel[g] = (uint8_t)ng;
    }
    carry += tot;
  }
}

// symbol counts per table under the current selectors (Bzip2:2043-2048) of symbols [i_lo, i_hi) (i_lo a multiple of 8) into
// eight replicas of [6][260] counters in `stage` (zeroed here): MTF output is dominated by a few symbols, the replicas (by
// lane) keep the same-address LDS atomics apart; the caller sums them
__device__ void count_symbols(uint32_t* __restrict__ stage, const uint16_t* __restrict__ A, const uint8_t* __restrict__ sel,
                              uint32_t npos, uint32_t i_lo, uint32_t i_hi) {
  for (int i = threadIdx.x; i < 8 * MAXTAB * FREQ_W; i += 1024) stage[i] = 0;
  __syncthreads();
  {
    uint32_t* rep = stage + (threadIdx.x & 7u) * (MAXTAB * FREQ_W);
    const uint4* A128 = reinterpret_cast<const uint4*>(A);                          // 8 symbols per load, two loads in flight
    const uint32_t nv = (i_hi < npos ? i_hi : npos) / 8;
    for (uint32_t v = i_lo / 8 + threadIdx.x; v < nv; v += 2048) {
      const uint32_t v2 = v + 1024;
      const uint4 x = A128[v];
      const uint4 y = v2 < nv ? A128[v2] : make_uint4(0, 0, 0, 0);
      const uint32_t i0 = v * 8, i1 = v2 * 8;
      const uint32_t ga = i0 / GSZ, gb = (i0 + 7) / GSZ, gc = v2 < nv ? i1 / GSZ : 0u, gd = v2 < nv ? (i1 + 7) / GSZ : 0u;
      const uint32_t sa = sel[ga], sb = sel[gb], sc = sel[gc], sd = sel[gd];
      const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t e0 = i0 + 2 * q, e1 = e0 + 1;
        atomicAdd(&rep[(e0 / GSZ == ga ? sa : sb) * FREQ_W + (xs[q] & 0xFFFFu)], 1u);
        atomicAdd(&rep[(e1 / GSZ == ga ? sa : sb) * FREQ_W + (xs[q] >> 16)], 1u);
      }
      if (v2 < nv) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint32_t e0 = i1 + 2 * q, e1 = e0 + 1;
          atomicAdd(&rep[(e0 / GSZ == gc ? sc : sd) * FREQ_W + (ys[q] & 0xFFFFu)], 1u);
          atomicAdd(&rep[(e1 / GSZ == gc ? sc : sd) * FREQ_W + (ys[q] >> 16)], 1u);
        }
      }
    }
    if (i_hi >= npos) for (uint32_t i = nv * 8 + threadIdx.x; i < npos; i += 1024) atomicAdd(&rep[sel[i / GSZ] * FREQ_W + A[i]], 1u);
  }
}

// bit accounting of a block whose tables (S.lens) and selectors are final: tile offsets of the symbol data, selector MTF
// positions, table bits, used-map bits, canonical codes, the block's bit length
__device__ void block_accounting(HuffShared& S, HuffBufs& hb, uint32_t blk, const uint8_t* __restrict__ sel, uint8_t* __restrict__ selj,
                                 const uint16_t* __restrict__ bcost, const uint8_t* __restrict__ alist_all, uint32_t nsel, uint32_t asz, int n, int ng) {
  // ---- bit accounting
  // data bits, and the bit offset of every 80-group tile inside the data (the tiles are packed in parallel)
  uint32_t data_bits = 0;
  {
    const uint32_t ntile = tiles_for_groups(nsel);                     // <= 226
    uint32_t tsum = 0;
    if (threadIdx.x < ntile) {
      const uint32_t g1 = (threadIdx.x + 1) * PD_GROUPS < nsel ? (threadIdx.x + 1) * PD_GROUPS : nsel;
      for (uint32_t g = threadIdx.x * PD_GROUPS; g < g1; g++) tsum += bcost[g];
    }
    const uint32_t tex = block_excl_sum<1024>(tsum, S.sm, data_bits);
    if (threadIdx.x < ntile) hb.tileoff[(size_t)blk * hb.tile_stride + threadIdx.x] = tex;
  }
  // selector MTF positions (Bzip2:2170-2182): j = #values more recent than the previous occurrence
  uint32_t sel_bits = 0;
  {
    uint32_t lastc[6] = {0, 0, 0, 0, 0, 0};                   // (last index+1) of each value in earlier tiles
    for (uint32_t base = 0; base < nsel; base += 1024) {
      const uint32_t g = base + threadIdx.x;
      const uint32_t sv = g < nsel ? sel[g] : 255u;
      uint32_t lastv[6];
#pragma unroll
      for (int v = 0; v < 6; v++) {
        const uint32_t mine = sv == (uint32_t)v ? g + 1 : 0u;
        const uint32_t im = block_incl_max<1024>(mine, S.sm);
        S.chist[threadIdx.x] = im;
        __syncthreads();
        const uint32_t ex = threadIdx.x ? S.chist[threadIdx.x - 1] : 0u;
        const uint32_t tmax = S.chist[1023];
        __syncthreads();
        lastv[v] = ex > lastc[v] ? ex : lastc[v];
        lastc[v] = tmax > lastc[v] ? tmax : lastc[v];
      }
      if (g < nsel) {
        uint32_t j = 0, mylast = 0;
#pragma unroll
        for (int v = 0; v < 6; v++) if ((uint32_t)v == sv) mylast = lastv[v];
#pragma unroll
        for (int v = 0; v < 6; v++) {
          if (v >= ng || (uint32_t)v == sv) continue;
          if (mylast) j += lastv[v] > mylast;                 // seen before: values touched since then
          else j += (lastv[v] != 0) || ((uint32_t)v < sv);    // first use: seen values + unseen smaller ones
        }
        selj[g] = (uint8_t)j;
        sel_bits += selector_item(j).nbits;
      }
    }
  }
  sel_bits = block_sum<1024>(sel_bits, S.sm);
  uint32_t tab_bits = 0;
  for (int i = threadIdx.x; i < ng * n; i += 1024) {                                // Bzip2:1926-1947
    const int t = i / n, s = i - t * n;
    const int cur = S.lens[t][s], prev = s ? S.lens[t][s - 1] : cur;
    tab_bits += table_item((uint32_t)cur, (uint32_t)prev, s == 0).nbits;
  }
  tab_bits = block_sum<1024>(tab_bits, S.sm);
  // used map: 16 + 16 per non-empty range (Bzip2:2071-2080)
  if (threadIdx.x < 8) S.counts[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x < asz) atomicOr(&S.counts[0], 1u << (alist_all[(size_t)blk * 256 + threadIdx.x] >> 4));
  __syncthreads();
  const uint32_t nranges = (uint32_t)__builtin_popcount(S.counts[0]);
  // canonical codes (Bzip2:1896-1916): code = first_code[len] + #{smaller symbols with the same len}
  uint8_t* glens = hb.lens + (size_t)blk * lens_row_bytes();
  uint32_t* gcodes = hb.codes + (size_t)blk * codes_row_elems();
  for (int i = threadIdx.x; i < 6 * 32; i += 1024) (&S.key[0][0])[i] = 0;           // reuse key[] as len histograms [6][32]
  __syncthreads();
  uint32_t* lhist = &S.key[0][0];
  for (int i = threadIdx.x; i < ng * n; i += 1024) { const int t = i / n, s = i - t * n; atomicAdd(&lhist[t * 32 + S.lens[t][s]], 1u); }
  __syncthreads();
  if (threadIdx.x < (uint32_t)ng) {
    canon_first_codes(lhist + threadIdx.x * 32, (uint32_t*)&S.work[0][0] + threadIdx.x * 32);      // first code per length
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ng * n; i += 1024) {
    const int t = i / n, s = i - t * n;
    const int l = S.lens[t][s];
    gcodes[t * MAXSYM + s] = ((const uint32_t*)&S.work[0][0])[t * 32 + l] + canon_rank(S.lens[t], s);
    glens[t * MAXSYM + s] = (uint8_t)l;
  }
  if (threadIdx.x == 0) {
    hb.ngroups[blk] = (uint32_t)ng;
    hb.bitlen[blk] = block_bits(nranges, sel_bits, tab_bits, data_bits);
    hb.databits[blk] = data_bits;
  }
}

__global__ __launch_bounds__(1024) void huff_block(HuffBufs hb, const uint16_t* __restrict__ Aall, size_t a_stride,
                                                   const uint32_t* __restrict__ npos_all, const uint32_t* __restrict__ asz_all,
                                                   const uint32_t* __restrict__ freq_all, const uint8_t* __restrict__ alist_all, int dbg) {
  __shared__ HuffShared S;
  __shared__ uint32_t stage[AS_GROUPS * 25];
  const uint32_t blk = blockIdx.x;
  const uint32_t npos = npos_all[blk], asz = asz_all[blk];
  const int n = (int)asz + 2;
  const uint16_t* A = Aall + (size_t)blk * a_stride;
  uint8_t* sel = hb.sel + (size_t)blk * hb.sel_stride;
  uint8_t* selj = hb.selj + (size_t)blk * hb.sel_stride;
  uint16_t* bcost = hb.bcost + (size_t)blk * hb.sel_stride;
  const uint32_t nsel = groups_for(npos);
  const int target = huff_target(npos);
  const int w = wave_id();

  HB_MARK(0);
  // initial tables: global frequencies and flat (Bzip2:2155-2157)
  for (int i = threadIdx.x; i < n; i += 1024) { S.freq[0][i] = freq_all[(size_t)blk * MAXSYM + i]; S.freq[1][i] = 1; }
  __syncthreads();
  if (w < 2) build_table_wave(S.freq[w], S.lens[w], S.key[w], S.work[w], n);
  __syncthreads();
  int ng = 2;
  HB_MARK(1);
  while (ng < target) {                                                             // Bzip2:2012-2053
    assign_selectors(S, stage, A, npos, nsel, ng, sel, bcost);
    if (ng == 2) HB_MARK(2);
    median_split(S, sel, bcost, nsel, ng);
    if (ng == 2) HB_MARK(3);
    ng++;
    count_symbols(stage, A, sel, npos, 0u, npos);
    __syncthreads();
    for (int i = threadIdx.x; i < MAXTAB * FREQ_W; i += 1024) {
      uint32_t f = 0;
#pragma unroll
      for (int r = 0; r < 8; r++) f += stage[r * (MAXTAB * FREQ_W) + i];
      (&S.freq[0][0])[i] = f;
    }
    __syncthreads();
    if (ng == 3) HB_MARK(4);
    if (w < ng) build_table_wave(S.freq[w], S.lens[w], S.key[w], S.work[w], n);
    __syncthreads();
    if (ng == 3) HB_MARK(5);
  }
  HB_MARK(6);
  assign_selectors(S, stage, A, npos, nsel, ng, sel, bcost);                        // Bzip2:2163
  __syncthreads();

  HB_MARK(7);
  block_accounting(S, hb, blk, sel, selj, bcost, alist_all, nsel, asz, n, ng);
  HB_MARK(8);
  HB_MARK(9);
}

// ------------------------------------------------------------------ the same refinement as a chain of kernels
// huff_block keeps one CU per block busy for ~0.9 ms while the other CUs idle (a -9 call of 100 MB has 112 blocks).  Its
// per-group and per-symbol phases (selector assignment, symbol counts) are data-parallel, so here they are kernels of
// their own with many workgroups per block; the per-block phases (median split, table builds, accounting) stay one
// workgroup per block.  State between the kernels: code lengths wl[blk][6][264], counts wfreq[blk][6][260].
// ng = tables in use when the kernel runs; a block takes part while ng <= / < its target (Bzip2:2150).
__device__ __forceinline__ void load_lens(HuffShared& S, const uint8_t* __restrict__ wl, int ng) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(wl);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&S.lens[0][0]);
  for (int i = threadIdx.x; i < ng * (WL_W / 4); i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}
__global__ __launch_bounds__(128) void hs_init(HuffBufs hb, const uint32_t* __restrict__ asz_all, const uint32_t* __restrict__ freq_all) {
  __shared__ uint32_t freq[2][FREQ_W], key[2][FREQ_W];
  __shared__ int work[2][FREQ_W];
  __shared__ uint8_t lens[2][WL_W];
  const uint32_t blk = blockIdx.x;
  const int n = (int)asz_all[blk] + 2, w = wave_id();
  for (int i = threadIdx.x; i < n; i += 128) { freq[0][i] = freq_all[(size_t)blk * MAXSYM + i]; freq[1][i] = 1; }
  __syncthreads();
  build_table_wave(freq[w], lens[w], key[w], work[w], n);
  __syncthreads();
  uint8_t* wl = hb.wl + (size_t)blk * wl_row_bytes();
  for (int i = threadIdx.x; i < 2 * WL_W; i += 128) wl[i] = (&lens[0][0])[i];
}
__global__ __launch_bounds__(1024) void hs_assign(HuffBufs hb, const uint16_t* __restrict__ Aall, size_t a_stride, const uint32_t* __restrict__ npos_all, int ng) {
  __shared__ HuffShared S;
  __shared__ uint32_t stage[AS_GROUPS * 25];
  const uint32_t blk = blockIdx.y, npos = npos_all[blk], nsel = groups_for(npos);
  const uint32_t g_lo = blockIdx.x * (HS_STEPS * AS_GROUPS);
  if (ng > huff_target(npos) || g_lo >= nsel) return;
  load_lens(S, hb.wl + (size_t)blk * wl_row_bytes(), ng);
  assign_selectors(S, stage, Aall + (size_t)blk * a_stride, npos, nsel, ng, hb.sel + (size_t)blk * hb.sel_stride, hb.bcost + (size_t)blk * hb.sel_stride,
                   g_lo, g_lo + HS_STEPS * AS_GROUPS);
}
__global__ __launch_bounds__(1024) void hs_split(HuffBufs hb, const uint32_t* __restrict__ npos_all, int ng) {
  __shared__ HuffShared S;
  const uint32_t blk = blockIdx.x, npos = npos_all[blk], nsel = groups_for(npos);
  if (ng >= huff_target(npos)) return;
  median_split(S, hb.sel + (size_t)blk * hb.sel_stride, hb.bcost + (size_t)blk * hb.sel_stride, nsel, ng);
  uint32_t* wf = hb.wfreq + (size_t)blk * wfreq_row_elems();
  for (int i = threadIdx.x; i < MAXTAB * FREQ_W; i += 1024) wf[i] = 0;
}
__global__ __launch_bounds__(1024) void hs_count(HuffBufs hb, const uint16_t* __restrict__ Aall, size_t a_stride, const uint32_t* __restrict__ npos_all, int ng) {
  __shared__ uint32_t stage[8 * MAXTAB * FREQ_W];
  const uint32_t blk = blockIdx.y, npos = npos_all[blk];
  const uint32_t i_lo = blockIdx.x * HS_CNT;
  if (ng >= huff_target(npos) || i_lo >= npos) return;
  count_symbols(stage, Aall + (size_t)blk * a_stride, hb.sel + (size_t)blk * hb.sel_stride, npos, i_lo, i_lo + HS_CNT);
  __syncthreads();
  uint32_t* wf = hb.wfreq + (size_t)blk * wfreq_row_elems();
  for (int i = threadIdx.x; i < MAXTAB * FREQ_W; i += 1024) {
    uint32_t f = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) f += stage[r * (MAXTAB * FREQ_W) + i];
    if (f) atomicAdd(&wf[i], f);
  }
}
__global__ __launch_bounds__(384) void hs_build(HuffBufs hb, const uint32_t* __restrict__ npos_all, const uint32_t* __restrict__ asz_all, int ng /* before the new table */) {
  __shared__ uint32_t freq[MAXTAB][FREQ_W], key[MAXTAB][FREQ_W];
  __shared__ int work[MAXTAB][FREQ_W];
  __shared__ uint8_t lens[MAXTAB][WL_W];
  const uint32_t blk = blockIdx.x, npos = npos_all[blk];
  if (ng >= huff_target(npos)) return;
  const int n = (int)asz_all[blk] + 2, w = wave_id();
  const uint32_t* wf = hb.wfreq + (size_t)blk * wfreq_row_elems();
  for (int i = threadIdx.x; i < MAXTAB * FREQ_W; i += 384) (&freq[0][0])[i] = wf[i];
  __syncthreads();
  if (w <= ng) build_table_wave(freq[w], lens[w], key[w], work[w], n);
  __syncthreads();
  uint8_t* wl = hb.wl + (size_t)blk * wl_row_bytes();
  for (int i = threadIdx.x; i < (ng + 1) * WL_W; i += 384) wl[i] = (&lens[0][0])[i];
}
__global__ __launch_bounds__(1024) void hs_finish(HuffBufs hb, const uint32_t* __restrict__ npos_all, const uint32_t* __restrict__ asz_all,
                                                  const uint8_t* __restrict__ alist_all) {
  __shared__ HuffShared S;
  const uint32_t blk = blockIdx.x, npos = npos_all[blk], asz = asz_all[blk], nsel = groups_for(npos);
  const int ng = huff_target(npos);
  load_lens(S, hb.wl + (size_t)blk * wl_row_bytes(), ng);
  block_accounting(S, hb, blk, hb.sel + (size_t)blk * hb.sel_stride, hb.selj + (size_t)blk * hb.sel_stride, hb.bcost + (size_t)blk * hb.sel_stride,
                   alist_all, nsel, asz, (int)asz + 2, ng);
}

int huff_tables_run(hipStream_t s, HuffWork& w, uint32_t nb, const SymRows& r, int path) {
  if (nb == 0) return 0;
  if (path != HUFF_AUTO && path != HUFF_PER_BLOCK && path != HUFF_CHAIN) return CJS_E_INVALID_ARG;
  const bool dbg = env_debug();
  // one workgroup per block (huff_block) keeps nb CUs busy; with fewer blocks than CUs the chain of kernels spreads the
  // data-parallel phases over the whole chip
  const bool split = path == HUFF_AUTO ? nb >= 8 && nb <= 512 && (size_t)nb * w.max_stride >= ((size_t)8 << 20) : path == HUFF_CHAIN;
  if (split) {
    const uint32_t ga = hs_assign_grid(w.max_stride), gc = hs_count_grid(w.max_stride);
    hipLaunchKernelGGL(hs_init, dim3(nb), dim3(128), 0, s, w.b, r.asz, r.freq);
    for (int ng = 2; ng <= 6; ng++) {
      hipLaunchKernelGGL(hs_assign, dim3(ga, nb), dim3(1024), 0, s, w.b, r.A, r.a_stride, r.npos, ng);
      if (ng == 6) break;
      hipLaunchKernelGGL(hs_split, dim3(nb), dim3(1024), 0, s, w.b, r.npos, ng);
      hipLaunchKernelGGL(hs_count, dim3(gc, nb), dim3(1024), 0, s, w.b, r.A, r.a_stride, r.npos, ng);
      hipLaunchKernelGGL(hs_build, dim3(nb), dim3(384), 0, s, w.b, r.npos, r.asz, ng);
    }
    hipLaunchKernelGGL(hs_finish, dim3(nb), dim3(1024), 0, s, w.b, r.npos, r.asz, r.alist);
    CJS_HIP_TRY(hipGetLastError());
    if (dbg) {
      uint64_t clk[8];
      CJS_HIP_TRY(hipStreamSynchronize(s));
      CJS_HIP_TRY(hipMemcpyFromSymbol(clk, HIP_SYMBOL(g_bt_clk), sizeof clk));
      fprintf(stderr, "[cjs huff] last table build of block 0 / wave 0: rank sort %.1f us, allocator pass 1 %.1f, pass 2 %.1f, pass 3 %.1f, lengths back %.1f us\n",
              (double)(clk[1] - clk[0]) / 100.0, (double)(clk[2] - clk[1]) / 100.0, (double)(clk[3] - clk[2]) / 100.0, (double)(clk[5] - clk[3]) / 100.0, (double)(clk[6] - clk[5]) / 100.0);
    }
    return 0;
  }
  hipLaunchKernelGGL(huff_block, dim3(nb), dim3(1024), 0, s, w.b, r.A, r.a_stride, r.npos, r.asz, r.freq, r.alist, dbg ? 1 : 0);
  CJS_HIP_TRY(hipGetLastError());
  if (dbg) {
    uint64_t clk[32];
    CJS_HIP_TRY(hipStreamSynchronize(s));
    CJS_HIP_TRY(hipMemcpyFromSymbol(clk, HIP_SYMBOL(g_huff_clk), sizeof clk));
    static const char* names[] = {"init tables", "assign(ng=2)", "median split(ng=2)", "freq count(ng=2->3)", "build tables(ng=3)",
                                  "rest of refinement", "final assign", "bit accounting, codes"};
    for (int i = 0; i < 8; i++) fprintf(stderr, "[cjs huff] wg0 %-36s %8.1f us\n", names[i], (double)(clk[i + 1] - clk[i]) / 100.0);
  }
  return 0;
}

}  // namespace cjs
