// compare.hip -- compare for .bz2 streams (cjs_bzip2_compare[_device], cjs_bzip2_compare_streams[_device]): the fourth
// consumer of the pass engine of the indexed entry points (range_engine.h).  Every decoded inverse-BWT batch is compared with the
// other side where it stands expanded in device scratch; 16 bytes per reported difference leave the GPU.
//   cm_count   per 16 KiB tile of a segment: the byte positions where the two sides differ, and the lowest such decoded offset
//   cm_scan    the exclusive scan of the tile counts (one workgroup), the batch's total behind them; the minimum of the firsts
//   cm_emit    the differences of a tile again, written at base + rank
// A segment is a run of GOOD, index-consecutive blocks of a batch, clipped to the window and intersected with the runs of the
// other side: len bytes of the stream at one device address, the len bytes they are compared with at another.  The two addresses
// have independent alignment mod 16.  A difference is one byte: nothing spans a batch, so there is no carry.
#include "range_engine.h"
#include "prims.hpp"
#include <stdlib.h>
#include <string.h>

using namespace cjs;

namespace cjs {

constexpr uint32_t CM_TILE = 16384;                                        // bytes of a tile
constexpr uint32_t CM_ROWS = (15 + CM_TILE + 15) / 16 / 64 + 1;            // a row = the 64 vectors a wave looks at at once
static_assert(CM_ROWS <= 64, "the rows of a tile are scanned by one wave");

struct CmSeg { uint64_t a, b, len, off, tile0; };      // len bytes at device address a against those at b; decoded offset; first tile
// A tile: n bytes at a0 against n bytes at b0.  Vector v is the aligned 16 bytes at abase + 16 v of the stream's side; the other
// side's bytes for it start at bd + 16 v = 16 q + 4 K + m behind an aligned address, K and m the same for every vector of the tile.
struct CmTile { uint64_t a0, b0, off0, abase, bd; uint32_t n, nvec, K, m; };

__device__ __forceinline__ CmTile cm_tile(const CmSeg* __restrict__ segs, uint32_t nseg) {
  const uint64_t t = blockIdx.x;
  uint32_t lo = 0, hi = nseg;                                                // the last segment with tile0 <= t
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (segs[mid].tile0 <= t) lo = mid; else hi = mid; }
  const CmSeg g = segs[lo];
  const uint64_t p0 = (t - g.tile0) * CM_TILE;
  CmTile T;
  T.a0 = g.a + p0; T.b0 = g.b + p0; T.off0 = g.off + p0;
  T.n = (uint32_t)min((uint64_t)CM_TILE, g.len - p0);
  T.abase = T.a0 & ~15ull;
  T.nvec = ((uint32_t)(T.a0 & 15u) + T.n + 15u) / 16u;
  T.bd = T.b0 - (T.a0 & 15u);
  T.K = (uint32_t)(T.bd & 15u) >> 2; T.m = (uint32_t)(T.bd & 3u);
  return T;
}

// The 16 bytes of the other side at d = 16 q + 4 K + m: dword j is dwords K + j and K + j + 1 of the two aligned vectors that
// cover them, funnelled by m bytes.  Both loads are bounded to [lo, hi); bytes outside read as zeros.
template <int K>
__device__ __forceinline__ uint4 cm_funnel(uint64_t d, uint32_t m, uint64_t lo, uint64_t hi) {
  const uint64_t base = d & ~15ull;
  const uint4 a = rg_ld16(base, lo, hi);
  const uint4 b = (K || m) ? rg_ld16(base + 16, lo, hi) : make_uint4(0u, 0u, 0u, 0u);
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint4 o;
  o.x = __builtin_amdgcn_alignbyte(w[K + 1], w[K], m);
  o.y = __builtin_amdgcn_alignbyte(w[K + 2], w[K + 1], m);
  o.z = __builtin_amdgcn_alignbyte(w[K + 3], w[K + 2], m);
  o.w = __builtin_amdgcn_alignbyte(w[K + 4], w[K + 3], m);
  return o;
}

// Vector v of the tile: the stream's bytes and the other side's, in phase.  A byte outside the tile is zero on both sides.
__device__ __forceinline__ void cm_load(const CmTile& T, uint32_t v, uint4& a, uint4& b) {
  a = rg_ld16(T.abase + 16ull * v, T.a0, T.a0 + T.n);
  const uint64_t d = T.bd + 16ull * v, lo = T.b0, hi = T.b0 + T.n;
  switch (T.K) {                                                             // (the same for the whole workgroup)
    case 0: b = cm_funnel<0>(d, T.m, lo, hi); break;
    case 1: b = cm_funnel<1>(d, T.m, lo, hi); break;
    case 2: b = cm_funnel<2>(d, T.m, lo, hi); break;
    default: b = cm_funnel<3>(d, T.m, lo, hi); break;
  }
}

// bit 7 of every byte of x that is not zero
__device__ __forceinline__ uint32_t cm_nz4(uint32_t x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }
__device__ __forceinline__ uint32_t cm_count16(uint4 x) { return __popc(cm_nz4(x.x)) + __popc(cm_nz4(x.y)) + __popc(cm_nz4(x.z)) + __popc(cm_nz4(x.w)); }
// bit i = byte i of the 16 is not zero
__device__ __forceinline__ uint32_t cm_mask16(uint4 x) {
  auto nib = [](uint32_t z) { return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u); };
  return nib(cm_nz4(x.x)) | (nib(cm_nz4(x.y)) << 4) | (nib(cm_nz4(x.z)) << 8) | (nib(cm_nz4(x.w)) << 12);
}
__device__ __forceinline__ uint4 cm_xor(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ uint32_t cm_byte(uint4 x, uint32_t i) {
  const uint32_t w = (i >> 2) == 0 ? x.x : (i >> 2) == 1 ? x.y : (i >> 2) == 2 ? x.z : x.w;
  return (w >> (8 * (i & 3u))) & 0xFFu;
}

__global__ __launch_bounds__(256) void cm_count(const CmSeg* __restrict__ segs, uint32_t nseg, uint64_t* __restrict__ cnt, uint64_t* __restrict__ first) {
  __shared__ uint32_t sm[4], sm_min[4];
  const CmTile T = cm_tile(segs, nseg);
  uint32_t c = 0, pos = ~0u;                                                 // pos: the lane's lowest differing byte of the tile
  for (uint32_t v = threadIdx.x; v < T.nvec; v += 256) {
    uint4 a, b;
    cm_load(T, v, a, b);
    const uint4 x = cm_xor(a, b);
    const uint32_t k = cm_count16(x);
    c += k;
    if (k && pos == ~0u) pos = 16u * v + __builtin_ctz(cm_mask16(x)) - (uint32_t)(T.a0 & 15u);
  }
  const uint32_t total = block_sum<256, uint32_t>(c, sm);
  const uint32_t wmin = wave_min(pos);
  if (lane_id() == 0) sm_min[wave_id()] = wmin;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t lowest = min(min(sm_min[0], sm_min[1]), min(sm_min[2], sm_min[3]));
    cnt[blockIdx.x] = total;
    first[blockIdx.x] = lowest == ~0u ? ~0ull : T.off0 + lowest;
  }
}

// cnt[0 .. nt) -> their exclusive prefix sums, cnt[nt] = the total, cnt[nt + 1] = the minimum of first[0 .. nt)
__global__ __launch_bounds__(256) void cm_scan(uint64_t* __restrict__ cnt, const uint64_t* __restrict__ first, uint64_t nt) {
  __shared__ uint64_t sm[4];
  uint64_t run = 0, lowest = ~0ull;
  for (uint64_t b = 0; b < nt; b += 256) {
    const uint64_t i = b + threadIdx.x, v = i < nt ? cnt[i] : 0;
    if (i < nt) lowest = min(lowest, first[i]);
    uint64_t tot;
    const uint64_t ex = block_excl_sum<256, uint64_t>(v, sm, tot);
    if (i < nt) cnt[i] = run + ex;
    run += tot;
  }
  // (64-bit minimum of a wave: the lowest high word, then the lowest low word among the lanes that have it)
  const uint32_t hi = wave_min((uint32_t)(lowest >> 32)), lo = wave_min((uint32_t)(lowest >> 32) == hi ? (uint32_t)lowest : ~0u);
  if (lane_id() == 0) sm[wave_id()] = ((uint64_t)hi << 32) | lo;
  __syncthreads();
  if (threadIdx.x == 0) { cnt[nt] = run; cnt[nt + 1] = min(min(sm[0], sm[1]), min(sm[2], sm[3])); }
}

// Difference number `rank` of the batch (ranks ascend with the tile, the row, the lane and the byte: sorted by offset) goes to
// out[rank] if it is among the first `keep`.  No atomics: the ranks come from the scan, the row counts and the wave's prefix sums.
__global__ __launch_bounds__(256) void cm_emit(const CmSeg* __restrict__ segs, uint32_t nseg, const uint64_t* __restrict__ cnt, uint4* __restrict__ out, uint64_t keep) {
  __shared__ uint32_t row[64];
  const uint64_t base = cnt[blockIdx.x];
  if (cnt[blockIdx.x + 1] == base || base >= keep) return;
  if (threadIdx.x < 64) row[threadIdx.x] = 0;
  __syncthreads();
  const CmTile T = cm_tile(segs, nseg);
  for (uint32_t r = wave_id(); r * 64 < T.nvec; r += 4) {
    const uint32_t v = r * 64 + lane_id();
    uint32_t k = 0;
    if (v < T.nvec) { uint4 a, b; cm_load(T, v, a, b); k = cm_count16(cm_xor(a, b)); }
    const uint32_t s = wave_sum(k);
    if (lane_id() == 0) row[r] = s;
  }
  __syncthreads();
  if (wave_id() == 0) {                                                      // the rows' exclusive prefix sums
    const uint32_t k = row[lane_id()], inc = wave_incl_sum(k);
    row[lane_id()] = inc - k;
  }
  __syncthreads();
  for (uint32_t r = wave_id(); r * 64 < T.nvec; r += 4) {
    const uint32_t v = r * 64 + lane_id();
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (v < T.nvec) cm_load(T, v, a, b);
    uint32_t m = cm_mask16(cm_xor(a, b));
    const uint32_t k = __popc(m);
    uint64_t rank = base + row[r] + (wave_incl_sum(k) - k);
    const uint64_t o = T.off0 + 16ull * v - (T.a0 & 15u);
    for (; m && rank < keep; m &= m - 1, rank++) {
      const uint32_t i = __builtin_ctz(m);
      out[rank] = make_uint4((uint32_t)(o + i), (uint32_t)((o + i) >> 32), cm_byte(a, i) | (cm_byte(b, i) << 8), 0u);
    }
  }
}

}  // namespace cjs

// ---------------------------------------------------------------- the driver
namespace {

struct CmRun { uint64_t lo, hi, addr; };      // decoded bytes [lo, hi) of the other side at device address addr

// One pass of the engine over the blocks of the stream that [win_lo, win_hi) touches, against the other side: either `runs`
// (sorted, on the device) or `other` (host memory: other[k] is decoded byte other_lo + k; a batch uploads what its good blocks
// cover).  The list, the count, the first offset and the compared bytes go on from where the call stands.
struct CompareCall {
  const cjs_bz_index* ix = nullptr;
  uint64_t win_lo = 0, win_hi = 0;
  const std::vector<CmRun>* runs = nullptr;
  const uint8_t* other = nullptr; uint64_t other_lo = 0, other_hi = 0;
  cjs_bz_diff* diffs = nullptr; uint64_t cap = 0, n_diffs = 0, first = ~0ull, compared = 0;
  uint64_t h2d = 0, d2h = 0, tiles = 0, other_up = 0;

  int batch(const RangeBatch& B, const std::vector<uint8_t>& verdict) {
    hipStream_t s = B.s;
    std::vector<CmRun> mine;                                         // the stream's side: good blocks clipped to the window, neighbours merged
    for (size_t k = B.g0; k < B.g1; k++) {
      const uint32_t b = B.blk[k];
      if (verdict[b] != RG_GOOD) continue;
      const uint64_t o = ix->off[b], lo = std::max(o, win_lo), hi = std::min<uint64_t>(o + ix->e[b].size, win_hi);
      if (lo >= hi) continue;
      const uint64_t addr = (uint64_t)(uintptr_t)(B.d_exp + B.J.out_off[k]) + (lo - o);
      if (!mine.empty() && mine.back().hi == lo && mine.back().addr + (mine.back().hi - mine.back().lo) == addr) mine.back().hi = hi;
      else mine.push_back(CmRun{lo, hi, addr});
    }
    std::vector<CmRun> up;                                           // host form: the other side's bytes under `mine`, packed
    HostBuf staged; Owner<void*, PoolGive> d_other;
    uint64_t up_bytes = 0;
    int rc = 0;
    if (other) {
      uint64_t& bytes = up_bytes;
      for (const CmRun& r : mine) {
        const uint64_t lo = std::max(r.lo, other_lo), hi = std::min(r.hi, other_hi);
        if (lo < hi) { up.push_back(CmRun{lo, hi, bytes}); bytes += hi - lo; }
      }
      if (bytes) {
        staged = HostBuf((size_t)bytes); d_other = DevBuf((size_t)bytes + 64);
        if (!staged || !d_other.p) return CJS_E_OUT_OF_MEMORY;
        for (CmRun& r : up) { memcpy(staged.p + r.addr, other + (r.lo - other_lo), (size_t)(r.hi - r.lo)); r.addr += (uint64_t)(uintptr_t)d_other.p; }
      }
    }
    const std::vector<CmRun>& theirs = other ? up : *runs;
    std::vector<CmSeg> segs;
    uint64_t nt = 0, bytes = 0;
    for (const CmRun& r : mine) {
      auto it = std::upper_bound(theirs.begin(), theirs.end(), r.lo, [](uint64_t o, const CmRun& q) { return o < q.hi; });      // the first run that ends behind r.lo
      for (; it != theirs.end() && it->lo < r.hi; ++it) {
        const uint64_t lo = std::max(r.lo, it->lo), hi = std::min(r.hi, it->hi);
        if (lo >= hi) continue;
        segs.push_back(CmSeg{r.addr + (lo - r.lo), it->addr + (lo - it->lo), hi - lo, lo, nt});
        nt += (hi - lo + CM_TILE - 1) / CM_TILE; bytes += hi - lo;
      }
    }
    if (!nt) return hipStreamSynchronize(s) != hipSuccess ? (int)CJS_E_HIP : 0;
    if (nt > 0x7FFFFFFFull) { (void)hipStreamSynchronize(s); return CJS_E_UNSUPPORTED; }
    DevBuf d_segs(sizeof(CmSeg) * segs.size()), d_cnt(8 * (size_t)(nt + 2)), d_first(8 * (size_t)nt);
    if (!d_segs.p || !d_cnt.p || !d_first.p) { (void)hipStreamSynchronize(s); return CJS_E_OUT_OF_MEMORY; }
    const uint32_t nseg = (uint32_t)segs.size();
    uint64_t res[2] = {0, ~0ull};                                    // the batch's total, its lowest differing offset
    // from here on no way out without a synchronize: the copies may still be reading `segs` / `staged`, writing `res`
    if (staged && hipMemcpyAsync(d_other.p, staged.p, (size_t)up_bytes, hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
    if (!rc && hipMemcpyAsync(d_segs.p, segs.data(), sizeof(CmSeg) * segs.size(), hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
    if (!rc) {
      hipLaunchKernelGGL(cm_count, dim3((unsigned)nt), dim3(256), 0, s, (const CmSeg*)d_segs.p, nseg, (uint64_t*)d_cnt.p, (uint64_t*)d_first.p);
      hipLaunchKernelGGL(cm_scan, dim3(1), dim3(256), 0, s, (uint64_t*)d_cnt.p, (const uint64_t*)d_first.p, nt);
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(res, (uint64_t*)d_cnt.p + nt, 16, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = CJS_E_HIP;
    if (rc) return rc;
    h2d += up_bytes; other_up += up_bytes;
    h2d += sizeof(CmSeg) * segs.size(); d2h += 16; tiles += nt;
    const uint64_t total = res[0];
    const uint64_t keep = n_diffs < cap ? std::min<uint64_t>(total, cap - n_diffs) : 0;
    if (keep) {                                                      // (a count query and an equal batch never get here: one kernel pass less)
      DevBuf d_out(16 * (size_t)keep);
      if (!d_out.p) return CJS_E_OUT_OF_MEMORY;
      hipLaunchKernelGGL(cm_emit, dim3((unsigned)nt), dim3(256), 0, s, (const CmSeg*)d_segs.p, nseg, (const uint64_t*)d_cnt.p, (uint4*)d_out.p, keep);
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(diffs + n_diffs, d_out.p, 16 * (size_t)keep, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
      if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = CJS_E_HIP;
      if (rc) return rc;
      d2h += 16 * keep;
    }
    n_diffs += total; first = std::min(first, res[1]); compared += bytes;
    return 0;
  }
};

// the blocks of non-zero size that overlap [lo, hi), hi <= total_bytes
std::vector<uint32_t> blocks_of(const cjs_bz_index* ix, uint64_t lo, uint64_t hi) {
  std::vector<uint32_t> t;
  if (lo < hi)
    for (size_t b = range_block_of(ix, lo); b < ix->e.size() && ix->off[b] < hi; b++) if (ix->e[b].size) t.push_back((uint32_t)b);
  return t;
}

struct BadBlocks { uint64_t n = 0, first = ~0ull; };
BadBlocks bad_among(const std::vector<uint32_t>& touched, const std::vector<uint8_t>& verdict) {
  BadBlocks r;
  for (uint32_t b : touched) if (verdict[b] != RG_GOOD) { if (!r.n++) r.first = b; }
  return r;
}

void info_clear(cjs_bz_cmp_info* info) {
  memset(info, 0, sizeof *info);
  info->first_diff = info->first_bad_block = info->first_bad_block_b = ~0ull;
}

int check_stream(const void* in, size_t n, const cjs_bz_index* idx) {
  if (!in && n) return CJS_E_INVALID_ARG;
  if (idx->stream_bytes != n) { set_detail("the index is of a stream of %llu bytes", (unsigned long long)idx->stream_bytes); return CJS_E_INVALID_ARG; }
  return 0;
}

int current_device(const cjs_opts* opts, int& dev) {
  CJS_TRY(select_device(opts));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CJS_E_NO_DEVICE;
  return 0;
}

// cjs_bzip2_compare[_device]: the other side is plain bytes, one run
int compare_core(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const uint8_t* other, const uint8_t* d_other, size_t other_n,
                 uint64_t other_off, uint64_t off, uint64_t len, cjs_bz_diff* diffs, size_t cap, cjs_bz_cmp_info* info, const cjs_opts* opts) {
  clear_detail();
  if (!idx || !info || (!(other ? (const void*)other : (const void*)d_other) && other_n) || (!diffs && cap)) return CJS_E_INVALID_ARG;
  CJS_TRY(check_stream(in ? (const void*)in : (const void*)d_in, n, idx));
  info_clear(info);
  const uint64_t total = idx->off.back(), end = off + len < off ? total : std::min<uint64_t>(off + len, total);
  const uint64_t other_end = other_off + other_n < other_off ? ~0ull : other_off + other_n;
  const uint64_t lo = std::max(off, other_off), hi = std::min(end, other_end);
  const std::vector<uint32_t> touched = blocks_of(idx, lo, hi);
  if (touched.empty()) return 0;
  int dev = 0;
  CJS_TRY(current_device(opts, dev));
  RestoreDevice restore{dev};
  if (d_in && (!on_device(d_in, dev) || !on_device(d_other, dev))) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  CompareCall C;
  const std::vector<CmRun> one(1, CmRun{other_off, other_end, (uint64_t)(uintptr_t)d_other});
  C.ix = idx; C.win_lo = lo; C.win_hi = hi; C.diffs = diffs; C.cap = cap;
  if (d_in) C.runs = &one;
  else { C.other = other; C.other_lo = other_off; C.other_hi = other_end; }
  std::vector<uint8_t> verdict(idx->e.size(), RG_GOOD); std::vector<uint32_t> crc_got(idx->e.size(), 0);
  RangeStats st;
  CJS_TRY(range_engine(in, d_in, idx, touched, verdict, crc_got, dev, st, [&](const RangeBatch& B) { return C.batch(B, verdict); }));
  info->n_diffs = C.n_diffs; info->first_diff = C.first; info->compared = C.compared; info->blocks_decoded = touched.size();
  const BadBlocks bad = bad_among(touched, verdict);
  info->n_bad_blocks = bad.n; info->first_bad_block = bad.first;
  if (bad.n) range_bad_detail(idx, (size_t)bad.first, verdict, crc_got);
  if (env_debug())
    fprintf(stderr, "[cjs compare] %s: window [%llu, %llu), %zu of %zu blocks touched, %llu bad, %u passes (%u row batches, %u inverse-BWT batches), 1 windows, "
            "%llu tiles, other side uploaded %llu B, H2D %llu D2H %llu (of these the compare's own: H2D %llu D2H %llu), %llu diffs, %llu compared\n",
            d_in ? "device" : "host", (unsigned long long)lo, (unsigned long long)hi, touched.size(), idx->e.size(), (unsigned long long)bad.n, st.passes, st.a_batches,
            st.b_batches, (unsigned long long)C.tiles, (unsigned long long)C.other_up, (unsigned long long)(st.h2d + C.h2d), (unsigned long long)(st.d2h + C.d2h),
            (unsigned long long)C.h2d, (unsigned long long)C.d2h, (unsigned long long)C.n_diffs, (unsigned long long)C.compared);
  return 0;
}

uint64_t compare_window_bytes() {      // (read at every call: tests run the several-window path at small sizes)
  const char* v = getenv("CJS_COMPARE_WINDOW_BYTES");
  const unsigned long long x = v ? strtoull(v, nullptr, 10) : 0;
  return x ? (uint64_t)x : 64ull << 20;
}

// cjs_bzip2_compare_streams[_device]: the other side is stream B, read window by window into one device buffer
int compare_streams_core(const uint8_t* a, const uint8_t* d_a, size_t na, const cjs_bz_index* idx_a, const uint8_t* b, const uint8_t* d_b, size_t nb,
                         const cjs_bz_index* idx_b, uint64_t off, uint64_t len, cjs_bz_diff* diffs, size_t cap, cjs_bz_cmp_info* info, const cjs_opts* opts) {
  clear_detail();
  if (!idx_a || !idx_b || !info || (!diffs && cap)) return CJS_E_INVALID_ARG;
  CJS_TRY(check_stream(a ? (const void*)a : (const void*)d_a, na, idx_a));
  CJS_TRY(check_stream(b ? (const void*)b : (const void*)d_b, nb, idx_b));
  info_clear(info);
  const bool device = !a;
  const uint64_t total = std::min(idx_a->off.back(), idx_b->off.back()), hi = off + len < off ? total : std::min<uint64_t>(off + len, total);
  if (off >= hi) return 0;
  int dev = 0;
  CJS_TRY(current_device(opts, dev));
  RestoreDevice restore{dev};
  if (device && (!on_device(d_a, dev) || !on_device(d_b, dev))) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  const uint64_t W = std::min(compare_window_bytes(), hi - off);
  DevBuf d_win((size_t)W + 64);
  if (!d_win.p) return CJS_E_OUT_OF_MEMORY;
  std::vector<uint8_t> verdict_a(idx_a->e.size(), RG_GOOD), verdict_b(idx_b->e.size(), RG_GOOD);
  std::vector<uint32_t> crc_a(idx_a->e.size(), 0), crc_b(idx_b->e.size(), 0);
  CompareCall C;
  C.ix = idx_a; C.diffs = diffs; C.cap = cap;
  RangeStats st_a, st_b;
  uint32_t windows = 0;
  for (uint64_t wlo = off; wlo < hi; wlo += W, windows++) {
    const uint64_t whi = std::min(hi, wlo + W < wlo ? hi : wlo + W);
    // ---- B's window into the buffer: one range per touched block, so a bad block fails only its own range
    const std::vector<uint32_t> tb = blocks_of(idx_b, wlo, whi);
    std::vector<uint64_t> r_off, r_len;
    for (uint32_t k : tb) {
      const uint64_t lo = std::max(idx_b->off[k], wlo), e = std::min<uint64_t>(idx_b->off[k] + idx_b->e[k].size, whi);
      r_off.push_back(lo); r_len.push_back(e - lo);
    }
    CJS_TRY(range_read_to_device(b, d_b, idx_b, r_off.data(), r_len.data(), r_off.size(), (uint8_t*)d_win.p, verdict_b, crc_b, dev, st_b));
    std::vector<CmRun> runs;                                         // the good ranges, neighbours merged; byte o of the window at d_win + (o - wlo)
    for (size_t i = 0; i < tb.size(); i++) {
      if (verdict_b[tb[i]] != RG_GOOD) continue;
      if (!runs.empty() && runs.back().hi == r_off[i]) runs.back().hi += r_len[i];
      else runs.push_back(CmRun{r_off[i], r_off[i] + r_len[i], (uint64_t)(uintptr_t)d_win.p + (r_off[i] - wlo)});
    }
    // ---- A's blocks of the window against those runs (B's read has returned: the engine is not re-entered)
    C.win_lo = wlo; C.win_hi = whi; C.runs = &runs;
    CJS_TRY(range_engine(a, d_a, idx_a, blocks_of(idx_a, wlo, whi), verdict_a, crc_a, dev, st_a, [&](const RangeBatch& B) { return C.batch(B, verdict_a); }));
  }
  const std::vector<uint32_t> ta = blocks_of(idx_a, off, hi), tb = blocks_of(idx_b, off, hi);
  info->n_diffs = C.n_diffs; info->first_diff = C.first; info->compared = C.compared; info->blocks_decoded = ta.size();
  const BadBlocks bad_a = bad_among(ta, verdict_a), bad_b = bad_among(tb, verdict_b);
  info->n_bad_blocks = bad_a.n; info->first_bad_block = bad_a.first;
  info->n_bad_blocks_b = bad_b.n; info->first_bad_block_b = bad_b.first;
  if (bad_a.n) range_bad_detail(idx_a, (size_t)bad_a.first, verdict_a, crc_a);
  else if (bad_b.n) range_bad_detail(idx_b, (size_t)bad_b.first, verdict_b, crc_b);
  if (env_debug())
    fprintf(stderr, "[cjs compare] %s streams: window [%llu, %llu), %zu of %zu blocks touched, %llu bad, %u passes (%u row batches, %u inverse-BWT batches), %u windows "
            "of %llu B (other stream: %zu of %zu blocks, %llu bad, %u passes), %llu tiles, other side uploaded 0 B, H2D %llu D2H %llu (of these the compare's own: "
            "H2D %llu D2H %llu), %llu diffs, %llu compared\n",
            device ? "device" : "host", (unsigned long long)off, (unsigned long long)hi, ta.size(), idx_a->e.size(), (unsigned long long)bad_a.n, st_a.passes,
            st_a.a_batches, st_a.b_batches, windows, (unsigned long long)W, tb.size(), idx_b->e.size(), (unsigned long long)bad_b.n, st_b.passes,
            (unsigned long long)C.tiles, (unsigned long long)(st_a.h2d + st_b.h2d + C.h2d), (unsigned long long)(st_a.d2h + st_b.d2h + C.d2h),
            (unsigned long long)C.h2d, (unsigned long long)C.d2h, (unsigned long long)C.n_diffs, (unsigned long long)C.compared);
  return 0;
}

}  // namespace

extern "C" int cjs_bzip2_compare(const uint8_t* in, size_t n, const cjs_bz_index* idx, const uint8_t* other, size_t other_n, uint64_t other_off, uint64_t off,
                                 uint64_t len, cjs_bz_diff* diffs, size_t cap, cjs_bz_cmp_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  return compare_core(in, nullptr, n, idx, other, nullptr, other_n, other_off, off, len, diffs, cap, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_compare_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const uint8_t* d_other, size_t other_n, uint64_t other_off,
                                        uint64_t off, uint64_t len, cjs_bz_diff* diffs, size_t cap, cjs_bz_cmp_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  return compare_core(nullptr, d_in, n, idx, nullptr, d_other, other_n, other_off, off, len, diffs, cap, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_compare_streams(const uint8_t* a, size_t na, const cjs_bz_index* idx_a, const uint8_t* b, size_t nb, const cjs_bz_index* idx_b,
                                         uint64_t off, uint64_t len, cjs_bz_diff* diffs, size_t cap, cjs_bz_cmp_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  return compare_streams_core(a, nullptr, na, idx_a, b, nullptr, nb, idx_b, off, len, diffs, cap, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_compare_streams_device(const uint8_t* d_a, size_t na, const cjs_bz_index* idx_a, const uint8_t* d_b, size_t nb, const cjs_bz_index* idx_b,
                                                uint64_t off, uint64_t len, cjs_bz_diff* diffs, size_t cap, cjs_bz_cmp_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  return compare_streams_core(nullptr, d_a, na, idx_a, nullptr, d_b, nb, idx_b, off, len, diffs, cap, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
