// tally.hip -- the frequency table of a list of line keys (cjs_keys_tally[_device]): which records occur how often,
// grouped, filtered and ordered on the GPU; only the groups asked for and four scalars leave it.  The rule is tally_plan.h (no HIP).
//   tl_words    per record: the sort word len << 32 | check, its index as the value
//   (radix_passes over the word, 64 bits)
//   tl_hashes   per sorted slot: the record's hash, gathered through the permutation
//   (radix_passes over the hash, 64 bits: with the first sort the stable sort by the whole record, the bad records last)
//   tl_heads    per sorted slot: 1 = its record differs from its predecessor's, 0 = it does not, 2 = a bad record; per tile of
//               TL_TILE slots the number of heads and of bad records
//   tl_scan     one workgroup: the tiles' counts -> their exclusive prefix sums, the totals into the call's scalars
//   tl_groups   per head: its slot, at the head's rank (the tile's scanned count + the rank in the tile)
//   tl_filter   per group: count = the distance to the next head (the last one: to the first bad record), kept or not by the
//               filter; per tile of groups the number kept and the largest count
//   tl_compact  per kept group, at its rank among the kept: first, count, the order word and the rank as its value
//   (radix_passes over the order word: 32 bits by first, 32 + the bits of the largest count by count)
//   tl_emit     the first cap groups in that order as 32-byte records, two aligned 16-byte stores each
// No atomics: every rank comes from a scan.  The host waits twice for scalars (the groups, then the kept groups and the largest
// count): the launches behind each are sized by them.
#include "cjs_internal.h"
#include "host.h"
#include "prims.hpp"
#include "dec_engine.h"      // on_device
#include "tally.h"

using namespace cjs;

namespace cjs {

// a record by two 8-byte loads (the array is 8-byte aligned, not always 16)
__device__ __forceinline__ cjs_bz_linekey tl_load(const cjs_bz_linekey* __restrict__ keys, uint32_t i) {
  const uint64_t* p = reinterpret_cast<const uint64_t*>(keys + i);
  const uint64_t a = p[0], b = p[1];
  cjs_bz_linekey k;
  k.hash = a; k.len = (uint32_t)b; k.check = (uint32_t)(b >> 32);
  return k;
}

__global__ __launch_bounds__(256) void tl_words(const cjs_bz_linekey* __restrict__ keys, uint32_t n, uint64_t* __restrict__ w, uint32_t* __restrict__ v) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  w[i] = tl_w1(tl_load(keys, (uint32_t)i));
  v[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void tl_hashes(const cjs_bz_linekey* __restrict__ keys, uint32_t n, const uint32_t* __restrict__ v, uint64_t* __restrict__ h) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  h[i] = reinterpret_cast<const uint64_t*>(keys + v[i])[0];
}

__global__ __launch_bounds__(256) void tl_heads(const cjs_bz_linekey* __restrict__ keys, uint32_t n, const uint32_t* __restrict__ v, uint8_t* __restrict__ flag,
                                                uint64_t* __restrict__ nhead, uint64_t* __restrict__ nbad) {
  __shared__ uint32_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * TL_TILE;
  uint32_t heads = 0, bad = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t i = base + (uint64_t)r * 256 + threadIdx.x;
    if (i >= n) continue;
    const cjs_bz_linekey k = tl_load(keys, v[i]);
    uint8_t f;
    if (lk_is_bad(k)) { f = 2; bad++; }
    else { f = i == 0 || !tl_equal(k, tl_load(keys, v[i - 1])); heads += f; }
    flag[i] = f;
  }
  const uint32_t h = block_sum<256, uint32_t>(heads, sm), b = block_sum<256, uint32_t>(bad, sm);
  if (threadIdx.x == 0) { nhead[blockIdx.x] = h; nbad[blockIdx.x] = b; }
}

// One workgroup: cnt[0 .. nt) -> their exclusive prefix sums, their total to scal[s_cnt]; aux[0 .. nt) summed (MAX: their maximum
// taken) into scal[s_aux].  (The house form of range_engine.h's rg_scan_counts, with the second array beside it.)
template <bool MAX>
__global__ __launch_bounds__(256) void tl_scan(uint64_t* __restrict__ cnt, const uint64_t* __restrict__ aux, uint64_t nt, uint64_t* __restrict__ scal,
                                               int s_cnt, int s_aux) {
  __shared__ uint64_t sm[4];
  __shared__ uint64_t sa[4];
  uint64_t run = 0, acc = 0;
  for (uint64_t b = 0; b < nt; b += 256) {
    const uint64_t i = b + threadIdx.x, c = i < nt ? cnt[i] : 0, a = i < nt ? aux[i] : 0;
    if (MAX) acc = a > acc ? a : acc; else acc += a;
    uint64_t tot;
    const uint64_t ex = block_excl_sum<256, uint64_t>(c, sm, tot);
    if (i < nt) cnt[i] = run + ex;
    run += tot;
  }
  const uint64_t all = MAX ? wave_max(acc) : wave_sum(acc);
  if (lane_id() == 0) sa[wave_id()] = all;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t r = sa[0];
    for (int w = 1; w < 4; w++) r = MAX ? (sa[w] > r ? sa[w] : r) : r + sa[w];
    scal[s_cnt] = run; scal[s_aux] = r;
  }
}

// this thread's flag of round r of its tile -> the number of set flags of the tile in front of it (rounds in slot order)
__device__ __forceinline__ uint32_t tl_rank(uint32_t f, uint32_t& run, uint32_t* sm) {
  uint32_t tot;
  const uint32_t ex = block_excl_sum<256, uint32_t>(f, sm, tot);
  const uint32_t r = run + ex;
  run += tot;
  return r;
}

__global__ __launch_bounds__(256) void tl_groups(const uint8_t* __restrict__ flag, uint32_t n, const uint64_t* __restrict__ nhead, uint32_t* __restrict__ gpos) {
  __shared__ uint32_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * TL_TILE;
  const uint64_t g0 = nhead[blockIdx.x];
  uint32_t run = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t i = base + (uint64_t)r * 256 + threadIdx.x;
    const uint32_t f = i < n && flag[i] == 1;
    const uint32_t rk = tl_rank(f, run, sm);
    if (f) gpos[g0 + rk] = (uint32_t)i;      // (g0 + rk < the number of heads <= n)
  }
}

// group g of nd: its count; n_good = the slot of the first bad record
__device__ __forceinline__ uint32_t tl_count(const uint32_t* __restrict__ gpos, uint64_t g, uint64_t nd, uint32_t n_good) {
  return (g + 1 < nd ? gpos[g + 1] : n_good) - gpos[g];
}

__global__ __launch_bounds__(256) void tl_filter(const uint32_t* __restrict__ gpos, uint64_t nd, uint32_t n_good, uint64_t min_count, uint64_t max_count,
                                               uint64_t* __restrict__ nkept, uint64_t* __restrict__ maxc) {
  __shared__ uint32_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * TL_TILE;
  uint32_t kept = 0, big = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t g = base + (uint64_t)r * 256 + threadIdx.x;
    if (g >= nd) continue;
    const uint32_t c = tl_count(gpos, g, nd, n_good);
    kept += tl_kept(c, min_count, max_count);
    big = c > big ? c : big;
  }
  const uint32_t k = block_sum<256, uint32_t>(kept, sm);
  const uint32_t m = wave_max(big);
  if (lane_id() == 0) sm[wave_id()] = m;
  __syncthreads();
  if (threadIdx.x == 0) { nkept[blockIdx.x] = k; maxc[blockIdx.x] = max(max(sm[0], sm[1]), max(sm[2], sm[3])); }
}

__global__ __launch_bounds__(256) void tl_compact(const uint32_t* __restrict__ gpos, const uint32_t* __restrict__ v, uint64_t nd, uint32_t n_good, uint64_t min_count,
                                                  uint64_t max_count, uint32_t order, const uint64_t* __restrict__ nkept, uint32_t* __restrict__ cfirst,
                                                  uint32_t* __restrict__ ccount, uint64_t* __restrict__ ow, uint32_t* __restrict__ ov) {
  __shared__ uint32_t sm[4];
  const uint64_t base = (uint64_t)blockIdx.x * TL_TILE;
  const uint64_t r0 = nkept[blockIdx.x];
  uint32_t run = 0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t g = base + (uint64_t)r * 256 + threadIdx.x;
    uint32_t c = 0, f = 0;
    if (g < nd) { c = tl_count(gpos, g, nd, n_good); f = tl_kept(c, min_count, max_count); }
    const uint32_t rk = tl_rank(f, run, sm);
    if (!f) continue;
    const uint64_t at = r0 + rk;              // (at < the number of kept groups <= nd)
    const uint32_t first = v[gpos[g]];
    cfirst[at] = first; ccount[at] = c;
    ow[at] = tl_order_word(order, first, c); ov[at] = (uint32_t)at;
  }
}

__global__ __launch_bounds__(256) void tl_emit(const cjs_bz_linekey* __restrict__ keys, const uint32_t* __restrict__ ov, const uint32_t* __restrict__ cfirst,
                                               const uint32_t* __restrict__ ccount, uint64_t m, uint64_t first_base, cjs_bz_tally* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const uint32_t at = ov[j], first = cfirst[at];
  const uint64_t* p = reinterpret_cast<const uint64_t*>(keys + first);
  const uint64_t a = p[0], b = p[1], f = first_base + first, c = ccount[at];
  uint4* o = reinterpret_cast<uint4*>(out + j);
  o[0] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
  o[1] = make_uint4((uint32_t)f, (uint32_t)(f >> 32), (uint32_t)c, (uint32_t)(c >> 32));
}

// The stages over d_keys[0 .. n), 0 < n <= TL_MAX_KEYS, on stream s.  sink(m, write): called once n_groups is known, with m =
// min(cap, n_groups) > 0; it names the device array of m records, write(d_out) launches the emit into it.
template <typename Sink>
int tally_stages(hipStream_t s, TallyWork& w, const cjs_bz_linekey* d_keys, uint32_t n, uint32_t order, uint64_t min_count, uint64_t max_count,
                 uint64_t first_base, size_t cap, cjs_tally_info* info, Sink sink) {
  const unsigned per = (unsigned)((n + 255) / 256), nt = (unsigned)TallyWork::tiles(n);
  uint64_t scal[TL_SCALARS] = {0, 0, 0, 0};
  int cur = 0;
  hipLaunchKernelGGL(tl_words, dim3(per), dim3(256), 0, s, d_keys, n, w.k[0], w.v[0]);
  CJS_TRY(radix_passes<uint64_t>(s, w.rs, w.k[0], w.v[0], w.k[1], w.v[1], cur, n, 0, 64));
  hipLaunchKernelGGL(tl_hashes, dim3(per), dim3(256), 0, s, d_keys, n, (const uint32_t*)w.v[cur], w.k[cur]);
  CJS_TRY(radix_passes<uint64_t>(s, w.rs, w.k[0], w.v[0], w.k[1], w.v[1], cur, n, 0, 64));
  const uint32_t* perm = w.v[cur];
  uint32_t* gpos = w.v[1 - cur];
  hipLaunchKernelGGL(tl_heads, dim3(nt), dim3(256), 0, s, d_keys, n, perm, w.flag, w.tcnt, w.taux);
  hipLaunchKernelGGL((tl_scan<false>), dim3(1), dim3(256), 0, s, w.tcnt, (const uint64_t*)w.taux, (uint64_t)nt, w.scal, (int)TL_N_DISTINCT, (int)TL_N_BAD);
  hipLaunchKernelGGL(tl_groups, dim3(nt), dim3(256), 0, s, (const uint8_t*)w.flag, n, (const uint64_t*)w.tcnt, gpos);
  int rc = hipGetLastError() != hipSuccess || hipMemcpyAsync(scal, w.scal, 8 * 2, hipMemcpyDeviceToHost, s) != hipSuccess ? CJS_E_HIP : 0;
  if ((rc = hipStreamSynchronize(s) != hipSuccess && !rc ? (int)CJS_E_HIP : rc)) return rc;
  const uint64_t nd = scal[TL_N_DISTINCT];
  info->n_bad = scal[TL_N_BAD]; info->n_distinct = nd;
  if (info->n_bad > n || nd > n - info->n_bad) return CJS_E_HIP;      // (what sizes the launches below is checked, not trusted)
  if (!nd) return 0;
  const uint32_t n_good = n - (uint32_t)info->n_bad;
  const unsigned gt = (unsigned)TallyWork::tiles(nd);
  hipLaunchKernelGGL(tl_filter, dim3(gt), dim3(256), 0, s, (const uint32_t*)gpos, nd, n_good, min_count, max_count, w.tcnt, w.taux);
  hipLaunchKernelGGL((tl_scan<true>), dim3(1), dim3(256), 0, s, w.tcnt, (const uint64_t*)w.taux, (uint64_t)gt, w.scal, (int)TL_N_GROUPS, (int)TL_MAX_COUNT);
  rc = hipGetLastError() != hipSuccess || hipMemcpyAsync(scal + 2, w.scal + 2, 8 * 2, hipMemcpyDeviceToHost, s) != hipSuccess ? CJS_E_HIP : 0;
  if ((rc = hipStreamSynchronize(s) != hipSuccess && !rc ? (int)CJS_E_HIP : rc)) return rc;
  const uint64_t ng = scal[TL_N_GROUPS];
  info->n_groups = ng; info->max_count = scal[TL_MAX_COUNT];
  if (ng > nd || info->max_count > n_good) return CJS_E_HIP;
  const uint64_t m = std::min<uint64_t>(cap, ng);
  if (!m) return 0;
  // the order sort goes through the two key buffers and through ov / the group positions' buffer, all free behind tl_compact
  uint64_t* ok[2] = {w.k[1 - cur], w.k[cur]};
  uint32_t* ovv[2] = {w.ov, gpos};
  hipLaunchKernelGGL(tl_compact, dim3(gt), dim3(256), 0, s, (const uint32_t*)gpos, perm, nd, n_good, min_count, max_count, order, (const uint64_t*)w.tcnt,
                     w.cfirst, w.ccount, ok[0], ovv[0]);
  int oc = 0;
  // (tl_order_bits is a whole number of digits: the bits above it, ~count's ones, are never sorted on)
  CJS_TRY(radix_passes<uint64_t>(s, w.rs, ok[0], ovv[0], ok[1], ovv[1], oc, (uint32_t)ng, 0, tl_order_bits(order, info->max_count)));
  const uint32_t* sorted = ovv[oc];
  rc = sink(m, [&](cjs_bz_tally* d_out) {
    hipLaunchKernelGGL(tl_emit, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, d_keys, sorted, (const uint32_t*)w.cfirst, (const uint32_t*)w.ccount, m,
                       first_base, d_out);
  });
  return !rc && hipGetLastError() != hipSuccess ? (int)CJS_E_HIP : rc;
}
// ... with the workspace from the pool; returns with s drained, on every path (the workspace goes back to the pool behind it)
template <typename Sink>
int tally_run(hipStream_t s, const cjs_bz_linekey* d_keys, uint32_t n, uint32_t order, uint64_t min_count, uint64_t max_count, uint64_t first_base, size_t cap,
              cjs_tally_info* info, Sink sink) {
  Arena arena;
  TallyWork w;
  int rc = arena.init_pooled(TallyWork::bytes_needed(n));
  if (!rc) rc = w.carve(arena, n);
  if (!rc) rc = tally_stages(s, w, d_keys, n, order, min_count, max_count, first_base, cap, info, sink);
  return hipStreamSynchronize(s) != hipSuccess && !rc ? (int)CJS_E_HIP : rc;
}

// (declared in tally.h)
int tally_to_host(hipStream_t s, TallyWork& w, const cjs_bz_linekey* d_keys, uint32_t n, uint32_t order, uint64_t min_count, uint64_t max_count,
                  uint64_t first_base, cjs_bz_tally* out, size_t cap, cjs_tally_info* info, cjs_bz_tally* d_stage) {
  Owner<void*, PoolGive> d_out;
  const int rc = tally_stages(s, w, d_keys, n, order, min_count, max_count, first_base, cap, info, [&](uint64_t m, auto write) {
    if (!d_stage) {
      d_out.reset(DevPool::take(sizeof(cjs_bz_tally) * (size_t)m));
      if (!(d_stage = (cjs_bz_tally*)d_out.p)) return (int)CJS_E_OUT_OF_MEMORY;
    }
    write(d_stage);
    return hipMemcpyAsync(out, d_stage, sizeof(cjs_bz_tally) * (size_t)m, hipMemcpyDeviceToHost, s) != hipSuccess ? (int)CJS_E_HIP : 0;
  });
  return hipStreamSynchronize(s) != hipSuccess && !rc ? (int)CJS_E_HIP : rc;
}

}  // namespace cjs

namespace {

int tally_checks(const void* keys, size_t n, uint32_t order, uint64_t min_count, uint64_t max_count, const void* out, size_t cap, cjs_tally_info* info) {
  clear_detail();
  if (!info || (!keys && n) || (!out && cap) || !tl_args_ok(order, min_count, max_count)) return CJS_E_INVALID_ARG;
  *info = cjs_tally_info{(uint64_t)n, 0, 0, 0, 0};
  return (uint64_t)n > TL_MAX_KEYS ? CJS_E_UNSUPPORTED : 0;
}

}  // namespace

extern "C" int cjs_keys_tally(const cjs_bz_linekey* keys, size_t n, uint32_t order, uint64_t min_count, uint64_t max_count, cjs_bz_tally* out, size_t cap,
                              cjs_tally_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(tally_checks(keys, n, order, min_count, max_count, out, cap, info));
  if (!n) return 0;
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  DevBuf d_keys(sizeof(cjs_bz_linekey) * n);
  if (!d_keys.p) return CJS_E_OUT_OF_MEMORY;
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  int rc = hipMemcpyAsync(d_keys.p, keys, sizeof(cjs_bz_linekey) * n, hipMemcpyHostToDevice, s) != hipSuccess ? CJS_E_HIP : 0;
  if (rc) { (void)hipStreamSynchronize(s); return rc; }
  Arena arena;
  TallyWork w;
  if (!(rc = arena.init_pooled(TallyWork::bytes_needed(n))) && !(rc = w.carve(arena, n)))
    rc = tally_to_host(s, w, (const cjs_bz_linekey*)d_keys.p, (uint32_t)n, order, min_count, max_count, 0, out, cap, info);
  else (void)hipStreamSynchronize(s);
  if (env_debug())
    fprintf(stderr, "[cjs tally] host keys: %zu keys, %llu bad, %llu distinct, %llu kept, H2D %zu D2H %zu\n", n, (unsigned long long)info->n_bad,
            (unsigned long long)info->n_distinct, (unsigned long long)info->n_groups, sizeof(cjs_bz_linekey) * n,
            8 * (size_t)TL_SCALARS + sizeof(cjs_bz_tally) * (size_t)std::min<uint64_t>(cap, info->n_groups));
  return rc;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_keys_tally_device(const cjs_bz_linekey* d_keys, size_t n, uint32_t order, uint64_t min_count, uint64_t max_count, cjs_bz_tally* d_out,
                                     size_t cap, cjs_tally_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  CJS_TRY(tally_checks(d_keys, n, order, min_count, max_count, d_out, cap, info));
  if (((uintptr_t)d_keys & 7u) || ((uintptr_t)d_out & 15u)) return CJS_E_INVALID_ARG;
  if (!n) return 0;
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  if (!on_device(d_keys, cd.dev) || (cap && !on_device(d_out, cd.dev))) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  Stream s;
  CJS_HIP_TRY(hipStreamCreate(s.put()));
  return tally_run(s, d_keys, (uint32_t)n, order, min_count, max_count, 0, cap, info, [&](uint64_t m, auto write) {
    write(d_out);
    return 0;
  });
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_stage_keys_tally(const cjs_bz_linekey* keys, size_t n, uint32_t order, uint64_t min_count, uint64_t max_count, cjs_bz_tally* out, size_t cap,
                                    cjs_tally_info* info) {
  CJS_GUARD_BEGIN
  return tl_tally_host(keys, n, order, min_count, max_count, out, cap, info);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_INVALID_ARG)
}
