// bwtc_model.hip — the adaptive models of BWTC.compressFile (J/BWTC_joined_.js:1698-1825) evaluated on the MI355X, one
// workgroup per block: the model (FenwickModel :1496-1661 for levels 6-9, DefSumModel :1327-1439 for levels 1-5) is rebuilt
// per block (:1791) and does not depend on the coder state, so each block yields its list of coder steps
// (sy_f, lt_f, tot_f | shift; bwtc_format.h) for the serial host coder of bwtc.hip.
#include "cjs_internal.h"
#include "host.h"
#include "prims.hpp"
#include "mtf.h"
#include "bwtc_format.h"
#include <algorithm>
#include <vector>

using namespace cjs;

namespace cjs {

constexpr uint32_t F_MAX = 0xFF00u, F_INC = 0x0100u;

// ---------------------------------------------------------------- FenwickModel evaluated 64 symbols at a time
// Between two rescales the model only counts: every coded symbol adds F_INC to its own frequency, and a symbol whose
// frequency is zero is announced by the escape symbol first.  So for a chunk of 64 symbols with NO rescale inside,
// everything a coder step needs is a prefix count over the chunk:
//   frequency of s at position j      = leaf(s) at the chunk start + F_INC * #{j' < j : s_j' = s}
//   cumulative frequency below s      = cum(s)  at the chunk start + F_INC * #{j' < j : s_j' < s}
//   total                             = root    at the chunk start + F_INC * (steps so far)
//   escape events                     = first occurrences of symbols whose frequency was zero at the chunk start
// The 64x64 relations are two 64-bit masks per lane (same symbol / smaller symbol), built with 64 readlanes; the counts
// are popcounts.  The position whose steps make the total reach F_MAX (rescale), and the rare "last unseen symbol"
// escape, are done one at a time by fm_serial on the same flat leaf array; the chunk continues behind them.
// The model is kept as flat leaves (packed hi = main count, lo = escape-context count, as in the reference's tree
// leaves) plus an exclusive prefix array rebuilt per chunk: no tree.
__device__ __forceinline__ void fm_build_cum(const uint32_t* leaf, uint32_t* cum, int ns) {
  const int lane = lane_id(), i0 = 5 * lane;
  uint32_t pre[5], sum = 0;
#pragma unroll
  for (int k = 0; k < 5; k++) { pre[k] = sum; sum += i0 + k < ns ? leaf[i0 + k] : 0u; }
  const uint32_t ex = wave_incl_sum(sum) - sum;
#pragma unroll
  for (int k = 0; k < 5; k++) if (i0 + k <= ns) cum[i0 + k] = ex + pre[k];        // cum[ns] = root
  __builtin_amdgcn_wave_barrier();
}
__device__ void fm_rescale(uint32_t* leaf, int ns, int e) {    // _rescale (:1623-1654) on the flat leaves; e = slot of the escape symbol
  const int lane = lane_id();
  bool esc_here = false;
  for (int i = lane; i < ns; i += 64) {
    if (i == e) continue;
    uint32_t prob = leaf[i];
    if (prob & 0xFFFFu) { esc_here = true; continue; }
    prob = (prob & 0xFFFEFFFEu) >> 1;
    if (prob == 0) { prob = 1u; esc_here = true; }
    leaf[i] = prob;
  }
  const bool no_escape = __ballot(esc_here) == 0ull;
  if (lane == 0) {
    uint32_t prob = leaf[e];
    prob = (prob & 0xFFFEFFFEu) >> 1;
    if (no_escape) prob = 0; else if (prob == 0) prob = 1u << 16;
    leaf[e] = prob;
  }
  __builtin_amdgcn_wave_barrier();
}
// encode(symbol) for ONE symbol (:1530-1571), any state: escape, last escape, rescales
__device__ void fm_serial(uint32_t* leaf, uint32_t* cum, int ns, int e, int symbol, uint64_t* out, uint32_t& n) {
  const int lane = lane_id();
  fm_build_cum(leaf, cum, ns);
  uint32_t root = __builtin_amdgcn_readfirstlane(cum[ns]);
  const uint32_t leafv = __builtin_amdgcn_readfirstlane(leaf[symbol]);
  const bool esc = (leafv >> 16) == 0;
  if (esc) {
    const uint32_t sy_raw = __builtin_amdgcn_readfirstlane(leaf[e]), lt = __builtin_amdgcn_readfirstlane(cum[e]);
    uint32_t update = F_INC << 16;
    if ((root & 0xFFFFu) == 1u) update = 0u - sy_raw;          // last escape: zero it out
    if (lane == 0) { out[n] = (uint64_t)(sy_raw >> 16) | ((uint64_t)(lt >> 16) << 16) | ((uint64_t)(root >> 16) << 32); leaf[e] = sy_raw + update; }
    n++;
    __builtin_amdgcn_wave_barrier();
    root += update;
    if ((root >> 16) >= F_MAX) fm_rescale(leaf, ns, e);
    fm_build_cum(leaf, cum, ns);
    root = __builtin_amdgcn_readfirstlane(cum[ns]);
    const uint32_t sy2 = __builtin_amdgcn_readfirstlane(leaf[symbol]), lt2 = __builtin_amdgcn_readfirstlane(cum[symbol]);
    if (lane == 0) { out[n] = (uint64_t)(sy2 & 0xFFFFu) | ((uint64_t)(lt2 & 0xFFFFu) << 16) | ((uint64_t)(root & 0xFFFFu) << 32); leaf[symbol] = sy2 + ((F_INC << 16) - 1u); }
    n++;
    __builtin_amdgcn_wave_barrier();
    root += (F_INC << 16) - 1u;
    if ((root >> 16) >= F_MAX) fm_rescale(leaf, ns, e);
  } else {
    const uint32_t lt = __builtin_amdgcn_readfirstlane(cum[symbol]);
    if (lane == 0) { out[n] = (uint64_t)(leafv >> 16) | ((uint64_t)(lt >> 16) << 16) | ((uint64_t)(root >> 16) << 32); leaf[symbol] = leafv + (F_INC << 16); }
    n++;
    __builtin_amdgcn_wave_barrier();
    root += F_INC << 16;
    if ((root >> 16) >= F_MAX) fm_rescale(leaf, ns, e);
  }
}

// The chunks of a block are a chain only through the model state (leaf counts, steps so far); the 64x64 relation masks of a
// chunk -- most of its instructions -- depend on nothing but its symbols.  FP_WAVES waves share a block: wave w takes the
// chunks w, w + FP_WAVES, ...; it builds its masks while the waves in front of it run their state parts, then waits for the
// baton (an LDS ticket), runs the state part of its chunk on the shared leaf array and passes the baton on.  A lone wave
// issues about one instruction per 8 cycles, so the block's critical path shrinks to the state parts alone.
constexpr int FP_WAVES = 8;
__global__ __launch_bounds__(64 * FP_WAVES) void bwtc_fenwick_par(MtfBufs mb, uint64_t* __restrict__ steps, size_t step_stride, uint32_t* __restrict__ nsteps) {
  __shared__ uint32_t leaf[328], cum[328];
  __shared__ uint32_t turn_s, n_s;           // next chunk whose state part may run; coder steps emitted so far
  const uint32_t blk = blockIdx.x;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t asz = mb.asz[blk], nsym = mb.npos[blk] - 1;      // drop bzip2's EOB
  const uint16_t* A = mb.A + (size_t)blk * mb.a_stride;
  uint64_t* out = steps + (size_t)blk * step_stride;
  const int lane = lane_id();
  const int ns = (int)asz + 2;
  // The reference keeps the counts in an implicit binary tree with the leaves at [ns, 2ns): "cumulative frequency below s"
  // is the sum over the leaves LEFT of s in that tree, and when ns is not a power of two the bottom-level leaves
  // (symbols >= r0) come first.  All slots below are in that order: slot(s) = (s - r0) mod ns.
  int dpt = 0; while ((2 << dpt) <= 2 * ns - 1) dpt++;                  // depth of the deepest leaf: floor(log2(2ns - 1))
  const int r0 = (1 << dpt) - ns, e = ns - 1 - r0;                      // slot of the escape symbol (symbol ns-1)
  for (int i = (int)threadIdx.x; i < 328; i += 64 * FP_WAVES) { leaf[i] = i == e ? (F_INC << 16) : i < ns ? 1u : 0u; cum[i] = 0; }
  if (threadIdx.x == 0) { turn_s = 0; n_s = 0; }
  __syncthreads();
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;       // lanes < lane
  const uint32_t nchunks = (nsym + 63u) / 64u;
  for (uint32_t ch = wv; ch < nchunks; ch += FP_WAVES) {
    const uint32_t base = ch * 64u;
    const uint32_t cnt = __builtin_amdgcn_readfirstlane(nsym - base < 64 ? nsym - base : 64);
    uint32_t mine = 0xFFFFu;
    if ((uint32_t)lane < cnt) { const int sy = (int)A[base + lane]; mine = (uint32_t)(sy >= r0 ? sy - r0 : sy + ns - r0); }
    const uint64_t LTE = __ballot(mine < (uint32_t)e);                  // positions whose slot lies left of the escape symbol
    // relations inside the chunk: lanes with the same / a smaller symbol (all 64 pairs, any window is a mask away)
    uint64_t eqm = 0, ltm = 0;
    for (uint32_t jp = 0; jp < cnt; jp++) {
      const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)jp);
      eqm |= sj == mine ? 1ull << jp : 0ull;
      ltm |= sj < mine ? 1ull << jp : 0ull;
    }
    // ---- the baton: everything below reads and writes the shared model state
    while ((uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&turn_s, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) != ch) __builtin_amdgcn_s_sleep(1);
    uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&n_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    uint32_t start = 0;
    while (start < cnt) {
      fm_build_cum(leaf, cum, ns);
      const uint32_t root = __builtin_amdgcn_readfirstlane(cum[ns]);
      const uint32_t esc_leaf = __builtin_amdgcn_readfirstlane(leaf[e]);
      const uint64_t win = (~0ull << start) & (cnt == 64 ? ~0ull : ((1ull << cnt) - 1ull));    // positions [start, cnt)
      const bool active = (win >> lane) & 1ull;
      const uint64_t before = below & win;                                                   // positions [start, lane)
      const uint32_t leafv = active ? leaf[mine] : 0x10000u;
      const uint32_t cumv = active ? cum[mine] : 0u;
      const uint32_t eqb = (uint32_t)__builtin_popcountll(eqm & before);
      const bool escj = active && (leafv >> 16) == 0 && eqb == 0;                            // first occurrence of a zero-count symbol
      const uint64_t ESCM = __ballot(escj);
      const uint32_t Eb = (uint32_t)__builtin_popcountll(ESCM & before);
      const uint32_t rel = (uint32_t)lane - start;
      const uint32_t through = rel + 1u + Eb + (escj ? 1u : 0u);                             // steps up to and including this position
      const uint32_t root_hi = root >> 16, root_lo = root & 0xFFFFu;
      const uint32_t kstar = root_hi >= F_MAX ? 1u : (F_MAX - root_hi + F_INC - 1u) / F_INC;  // the step after which the total reaches F_MAX
      const bool cut = active && (through >= kstar || (escj && root_lo - Eb == 1u));
      const uint64_t cutm = __ballot(cut);
      const uint32_t c = cutm ? (uint32_t)__builtin_ctzll(cutm) : cnt;                       // [start, c) in parallel, c one at a time
      const uint64_t parw = win & (c == 64 ? ~0ull : ((1ull << c) - 1ull));
      if ((parw >> lane) & 1ull) {
        const uint32_t tot = root_hi + F_INC * (rel + Eb);
        const uint32_t o = n + rel + Eb;
        if (escj) {
          const uint32_t esc_hi = (esc_leaf >> 16) + F_INC * Eb;
          const uint32_t cum_e = (uint32_t)__builtin_amdgcn_readfirstlane(cum[e]);      // (the builtin returns int: shift the unsigned copy)
          const uint32_t lt_e = (cum_e >> 16) + F_INC * (uint32_t)__builtin_popcountll(LTE & before);
          out[o] = (uint64_t)esc_hi | ((uint64_t)lt_e << 16) | ((uint64_t)tot << 32);
          const uint32_t lt_lo = (cumv & 0xFFFFu) - (uint32_t)__builtin_popcountll(ESCM & ltm & before);
          out[o + 1] = 1ull | ((uint64_t)lt_lo << 16) | ((uint64_t)(root_lo - Eb) << 32);
        } else {
          const uint32_t sy = (leafv >> 16) + F_INC * eqb;
          // counts left of this slot: earlier symbols in lower slots, and the escape symbol's own increments if it lies left
          const uint32_t lt = (cumv >> 16) + F_INC * ((uint32_t)__builtin_popcountll(ltm & before) + (mine > (uint32_t)e ? Eb : 0u));
          out[o] = (uint64_t)sy | ((uint64_t)lt << 16) | ((uint64_t)tot << 32);
        }
        // the last occurrence of a symbol inside [start, c) writes its new leaf (count so far, escape count 0)
        const uint64_t later = eqm & parw & ~below & ~(1ull << lane);
        if (!later) leaf[mine] = ((leafv >> 16) + F_INC * (eqb + 1u)) << 16;
      }
      const uint32_t nesc = (uint32_t)__builtin_popcountll(ESCM & parw);
      if (lane == 0 && nesc) leaf[e] = esc_leaf + ((F_INC * nesc) << 16);
      n += (c - start) + nesc;
      __builtin_amdgcn_wave_barrier();
      if (c < cnt) {
        fm_serial(leaf, cum, ns, e, __builtin_amdgcn_readlane((int)mine, (int)c), out, n);
        start = c + 1;
      } else start = cnt;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      __hip_atomic_store(&n_s, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_store(&turn_s, ch + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);      // (orders the leaf / n_s stores in front of it)
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) nsteps[blk] = n_s;
}

// ---------------------------------------------------------------- DefSumModel (levels 1-5), one lane per block
__global__ __launch_bounds__(64) void bwtc_defsum(MtfBufs mb, uint64_t* __restrict__ steps, size_t step_stride, uint32_t* __restrict__ nsteps) {
  __shared__ uint16_t prob[304], esc[304], upd[304];
  const uint32_t blk = blockIdx.x;
  if (threadIdx.x != 0) return;                         // tiny state, O(1) per symbol: serial on one lane
  const uint32_t asz = mb.asz[blk], nsym = mb.npos[blk] - 1;
  const uint16_t* A = mb.A + (size_t)blk * mb.a_stride;
  uint64_t* out = steps + (size_t)blk * step_stride;
  const int ns = (int)asz + 1;                          // numSyms = size; ESCAPE = ns
  for (int i = 0; i < 304; i++) { prob[i] = 0; esc[i] = 0; upd[i] = 0; }
  prob[ns + 1] = 256;
  for (int i = 0; i <= ns; i++) esc[i] = (uint16_t)i;
  int update_count = 0, update_thresh = 128;
  uint32_t n = 0;
  auto do_update = [&](int symbol) {                    // _update (:1359-1421), encoder side
    if (symbol == ns) {
      if (upd[symbol] >= 40) return;
      if (update_count >= update_thresh - 1) return;
    }
    upd[symbol]++; update_count++;
    if (update_count < update_thresh) return;
    int cum = 0, cum_esc = 0, odd = 0, i;
    esc[0] = 0; prob[0] = 0;
    for (i = 0; i < ns + 1; i++) {
      const int np = ((prob[i + 1] - prob[i]) >> 1) + upd[i];
      prob[i] = (uint16_t)cum; esc[i] = (uint16_t)cum_esc;
      if (np) { cum += np; odd += np & 1; } else cum_esc++;
    }
    prob[i] = (uint16_t)cum;
    update_thresh = 256 - (cum - odd) / 2;
    for (i = 0; i < ns + 1; i++) upd[i] = 0;
    upd[ns] = 1; update_count = 1;
  };
  for (uint32_t k = 0; k < nsym; k++) {
    int symbol = A[k];
    uint32_t lt = prob[symbol], sy = (uint32_t)prob[symbol + 1] - lt;
    if (sy) { out[n++] = STEP_SHIFT_FLAG | sy | ((uint64_t)lt << 16) | (8ull << 32); do_update(symbol); continue; }
    // escape (:1430-1438)
    { const uint32_t elt = prob[ns], esy = (uint32_t)prob[ns + 1] - elt;
      out[n++] = STEP_SHIFT_FLAG | esy | ((uint64_t)elt << 16) | (8ull << 32); do_update(ns); }
    lt = esc[symbol]; sy = (uint32_t)esc[symbol + 1] - lt;
    out[n++] = (uint64_t)sy | ((uint64_t)lt << 16) | ((uint64_t)esc[ns] << 32);
    do_update(symbol);
  }
  nsteps[blk] = n;
}

// the model evaluation of `nb` blocks as the compressor launches it: one workgroup per block, DefSumModel on one lane of one
// wave (levels 1-5), FenwickModel on FP_WAVES waves (levels 6-9).  Reads mb.A / a_stride / asz / npos only.
int bwtc_model_launch(hipStream_t s, bool fast, const MtfBufs& mb, uint32_t nb, uint64_t* d_steps, size_t step_stride, uint32_t* d_nsteps) {
  if (fast) hipLaunchKernelGGL(bwtc_defsum, dim3(nb), dim3(64), 0, s, mb, d_steps, step_stride, d_nsteps);
  else hipLaunchKernelGGL(bwtc_fenwick_par, dim3(nb), dim3(64 * FP_WAVES), 0, s, mb, d_steps, step_stride, d_nsteps);
  return hipGetLastError() != hipSuccess ? (int)CJS_E_HIP : 0;
}

}  // namespace cjs

// ---------------------------------------------------------------- stage-level entry point (tests)
// The model kernels on caller-made symbol blocks: what bwtc_batch_body launches behind mtf_run, on rows laid out as MtfWork
// carves them.  Of MtfBufs the kernels read A, a_stride, asz and npos (symbols + 1: the MTF stage counts bzip2's end-of-block).
extern "C" int cjs_stage_bwtc_model(const uint16_t* A, size_t a_stride, uint32_t nb, const uint32_t* nsym, const uint32_t* alphabet, int level,
                                    uint64_t* steps, size_t step_stride, uint32_t* nsteps, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(select_device(opts));
  if (!A || !nsym || !alphabet || !steps || !nsteps || nb == 0 || nb > (1u << 20) || a_stride == 0 || step_stride < 2 || level < 1 || level > 9) return CJS_E_INVALID_ARG;
  // what the kernels rely on: symbols index model arrays of asz + 2 slots, a block writes at most two steps per symbol
  uint32_t max_nsym = 1;
  for (uint32_t k = 0; k < nb; k++) {
    const uint32_t n = nsym[k], asz = alphabet[k];
    if (asz == 0 || asz > 256 || n > a_stride || n > 900000u || 2 * (size_t)n > step_stride) return CJS_E_INVALID_ARG;
    const uint16_t* a = A + (size_t)k * a_stride;
    for (uint32_t i = 0; i < n; i++) if (a[i] > asz) return CJS_E_INVALID_ARG;
    max_nsym = std::max(max_nsym, n);
  }
  const size_t das = MtfWork::a_stride_for(max_nsym), dss = 2 * das;      // rows as bwtc_batch_body sizes them
  Arena arena;
  CJS_TRY(arena.init(2 * das * nb + 8 * dss * nb + 12 * (size_t)nb + 65536));
  MtfBufs mb{};
  mb.A = arena.take<uint16_t>(das * nb); mb.a_stride = das;
  mb.asz = arena.take<uint32_t>(nb); mb.npos = arena.take<uint32_t>(nb);
  uint32_t* d_nsteps = arena.take<uint32_t>(nb);
  uint64_t* d_steps = arena.take<uint64_t>(dss * nb);
  if (!mb.A || !mb.asz || !mb.npos || !d_nsteps || !d_steps) return CJS_E_OUT_OF_MEMORY;
  std::vector<uint32_t> npos(nb);
  for (uint32_t k = 0; k < nb; k++) npos[k] = nsym[k] + 1;
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  CJS_HIP_TRY(hipMemsetAsync(mb.A, 0, 2 * das * nb, s));
  CJS_HIP_TRY(hipMemsetAsync(d_steps, 0, 8 * dss * nb, s));
  CJS_HIP_TRY(hipMemsetAsync(d_nsteps, 0, 4 * (size_t)nb, s));
  CJS_HIP_TRY(hipMemcpy2DAsync(mb.A, 2 * das, A, 2 * a_stride, 2 * (size_t)std::min<size_t>(max_nsym, a_stride), nb, hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(mb.asz, alphabet, 4 * (size_t)nb, hipMemcpyHostToDevice, s));
  CJS_HIP_TRY(hipMemcpyAsync(mb.npos, npos.data(), 4 * (size_t)nb, hipMemcpyHostToDevice, s));
  CJS_TRY(bwtc_model_launch(s, level <= 5, mb, nb, d_steps, dss, d_nsteps));
  CJS_HIP_TRY(hipMemcpyAsync(nsteps, d_nsteps, 4 * (size_t)nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipMemcpy2DAsync(steps, 8 * step_stride, d_steps, 8 * dss, 8 * std::min<size_t>(2 * (size_t)max_nsym, step_stride), nb, hipMemcpyDeviceToHost, s));
  CJS_HIP_TRY(hipStreamSynchronize(s));
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
