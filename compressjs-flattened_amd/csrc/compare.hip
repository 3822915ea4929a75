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
#include <stdlib.h>
#include <string.h>

using namespace cjs;

namespace cjs {

constexpr uint32_t CM_TILE = 16384;                                        // bytes of a tile
constexpr uint32_t CM_ROWS = (15 + CM_TILE + 15) / 16 / 64 + 1;            // a row = the 64 vectors a wave looks at at once
static_assert(CM_ROWS <= 64, "the rows of a tile are scanned by one wave");

struct CmSeg : RunPair {};      // (scan_plan.h; the kernels' own name for it: the host hands them an array of RunPair)
// A tile: the span A of the stream's side, n bytes at a0, against n bytes at b0.  Vector v is the aligned 16 bytes at A.base + 16 v;
// the other side's bytes for it start at bd + 16 v = 16 q + 4 K + m behind an aligned address, K and m the same for every vector of
// the tile.
struct CmTile { RgSpan A; uint64_t b0, off0, bd; uint32_t K, m; };

__device__ __forceinline__ CmTile cm_tile(const CmSeg* __restrict__ segs, uint32_t nseg) {
  const uint64_t t = blockIdx.x;
  const CmSeg g = rg_seg_of(segs, nseg, t);
  const uint64_t p0 = (t - g.tile0) * CM_TILE;
  const uint64_t a0 = g.a + p0;
  CmTile T;
  T.b0 = g.b + p0; T.off0 = g.off + p0;
  T.A = rg_span(a0, (uint32_t)min((uint64_t)CM_TILE, g.len - p0));
  T.bd = T.b0 - (T.A.a0 & 15u);
  T.K = (uint32_t)(T.bd & 15u) >> 2; T.m = (uint32_t)(T.bd & 3u);
  return T;
}

// Vector v of the tile: the stream's bytes and the other side's, in phase.  A byte outside the tile is zero on both sides.
__device__ __forceinline__ void cm_load(const CmTile& T, uint32_t v, uint4& a, uint4& b) {
  a = rg_vec(T.A, v);
  const uint64_t d = T.bd + 16ull * v, lo = T.b0, hi = T.b0 + T.A.n;
  switch (T.K) {                                                             // (the same for the whole workgroup)
    case 0: b = rg_funnel16<0>(d, T.m, lo, hi); break;
    case 1: b = rg_funnel16<1>(d, T.m, lo, hi); break;
    case 2: b = rg_funnel16<2>(d, T.m, lo, hi); break;
    default: b = rg_funnel16<3>(d, T.m, lo, hi); break;
  }
}

// bit 7 of every byte of x that is not zero
__device__ __forceinline__ uint32_t cm_nz4(uint32_t x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }
// the non-zero bytes of 16: their number, and bit i = byte i is one
__device__ __forceinline__ uint32_t cm_count16(uint4 x) { return rg_count16<cm_nz4>(x); }
__device__ __forceinline__ uint32_t cm_mask16(uint4 x) { return rg_mask16<cm_nz4>(x); }
__device__ __forceinline__ uint4 cm_xor(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ uint32_t cm_byte(uint4 x, uint32_t i) {
  const uint32_t w = (i >> 2) == 0 ? x.x : (i >> 2) == 1 ? x.y : (i >> 2) == 2 ? x.z : x.w;
  return (w >> (8 * (i & 3u))) & 0xFFu;
}

__global__ __launch_bounds__(256) void cm_count(const CmSeg* __restrict__ segs, uint32_t nseg, uint64_t* __restrict__ cnt, uint64_t* __restrict__ first) {
  __shared__ uint32_t sm[4], sm_min[4];
  const CmTile T = cm_tile(segs, nseg);
  uint32_t c = 0, pos = ~0u;                                                 // pos: the lane's lowest differing byte of the tile
  for (uint32_t v = threadIdx.x; v < T.A.nvec; v += 256) {
    uint4 a, b;
    cm_load(T, v, a, b);
    const uint4 x = cm_xor(a, b);
    const uint32_t k = cm_count16(x);
    c += k;
    if (k && pos == ~0u) pos = 16u * v + __builtin_ctz(cm_mask16(x)) - (uint32_t)(T.A.a0 & 15u);
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
  uint64_t lowest = ~0ull;
  const uint64_t run = rg_scan_counts(cnt, nt, sm, [&](uint64_t i) { lowest = min(lowest, first[i]); });
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
  for (uint32_t r = wave_id(); r * 64 < T.A.nvec; r += 4) {
    const uint32_t v = r * 64 + lane_id();
    uint32_t k = 0;
    if (v < T.A.nvec) { uint4 a, b; cm_load(T, v, a, b); k = cm_count16(cm_xor(a, b)); }
    const uint32_t s = wave_sum(k);
    if (lane_id() == 0) row[r] = s;
  }
  __syncthreads();
  if (wave_id() == 0) {                                                      // the rows' exclusive prefix sums
    const uint32_t k = row[lane_id()], inc = wave_incl_sum(k);
    row[lane_id()] = inc - k;
  }
  __syncthreads();
  for (uint32_t r = wave_id(); r * 64 < T.A.nvec; r += 4) {
    const uint32_t v = r * 64 + lane_id();
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (v < T.A.nvec) cm_load(T, v, a, b);
    uint32_t m = cm_mask16(cm_xor(a, b));
    const uint32_t k = __popc(m);
    uint64_t rank = base + row[r] + (wave_incl_sum(k) - k);
    const uint64_t o = T.off0 + 16ull * v - (T.A.a0 & 15u);
    for (; m && rank < keep; m &= m - 1, rank++) {
      const uint32_t i = __builtin_ctz(m);
      out[rank] = make_uint4((uint32_t)(o + i), (uint32_t)((o + i) >> 32), cm_byte(a, i) | (cm_byte(b, i) << 8), 0u);
    }
  }
}

}  // namespace cjs

// ---------------------------------------------------------------- the driver
namespace {

using CmRun = ScanRun;      // decoded bytes [lo, hi) of the other side at device address addr

// One pass of the engine over the blocks of the stream that [win_lo, win_hi) touches, against the other side: either `runs`
// (sorted, on the device) or `other` (host memory: other[k] is decoded byte other_lo + k; a batch uploads what its good blocks
// cover).  The list, the count, the first offset and the compared bytes go on from where the call stands.
struct CompareCall {
  const cjs_bz_index* ix = nullptr;
  uint64_t win_lo = 0, win_hi = 0;
  const std::vector<CmRun>* runs = nullptr;
  const uint8_t* other = nullptr; uint64_t other_lo = 0, other_hi = 0;
  cjs_bz_diff* diffs = nullptr; uint64_t cap = 0, n_diffs = 0, first = ~0ull, compared = 0;
  ScanStats st; uint64_t other_up = 0;

  int batch(const RangeBatch& B) {
    hipStream_t s = B.s;
    const std::vector<CmRun> mine = B.good_runs(ix->off, win_lo, win_hi);      // the stream's side
    std::vector<CmRun> up;                                           // host form: the other side's bytes under `mine`, packed
    HostBuf staged; Owner<void*, PoolGive> d_other;
    uint64_t up_bytes = 0;
    if (other) {
      for (const CmRun& r : mine) {
        const uint64_t lo = std::max(r.lo, other_lo), hi = std::min(r.hi, other_hi);
        if (lo < hi) { up.push_back(CmRun{lo, hi, up_bytes}); up_bytes += hi - lo; }
      }
      if (up_bytes) {
        staged = HostBuf((size_t)up_bytes); d_other = DevBuf((size_t)up_bytes + 64);
        if (!staged || !d_other.p) return drained(s, CJS_E_OUT_OF_MEMORY);
        for (CmRun& r : up) { memcpy(staged.p + r.addr, other + (r.lo - other_lo), (size_t)(r.hi - r.lo)); r.addr += (uint64_t)(uintptr_t)d_other.p; }
      }
    }
    const RunPairs P = intersect_runs(mine, other ? up : *runs, CM_TILE);
    const uint64_t nt = P.tiles;
    const uint32_t nseg = (uint32_t)P.segs.size();
    Owner<void*, PoolGive> d_segs, d_first;
    auto count_scan = [&](uint64_t* cnt) {
      d_segs = DevBuf(sizeof(RunPair) * P.segs.size()); d_first = DevBuf(8 * (size_t)nt);
      if (!d_segs.p || !d_first.p) return (int)CJS_E_OUT_OF_MEMORY;
      if ((staged && hipMemcpyAsync(d_other.p, staged.p, (size_t)up_bytes, hipMemcpyHostToDevice, s) != hipSuccess) ||
          hipMemcpyAsync(d_segs.p, P.segs.data(), sizeof(RunPair) * P.segs.size(), hipMemcpyHostToDevice, s) != hipSuccess) return (int)CJS_E_HIP;
      st.h2d += up_bytes + sizeof(RunPair) * P.segs.size(); other_up += up_bytes;
      hipLaunchKernelGGL(cm_count, dim3((unsigned)nt), dim3(256), 0, s, (const CmSeg*)d_segs.p, nseg, cnt, (uint64_t*)d_first.p);
      hipLaunchKernelGGL(cm_scan, dim3(1), dim3(256), 0, s, cnt, (const uint64_t*)d_first.p, nt);
      return 0;
    };
    auto emit = [&](const uint64_t* cnt, uint4* out, uint64_t keep) {
      hipLaunchKernelGGL(cm_emit, dim3((unsigned)nt), dim3(256), 0, s, (const CmSeg*)d_segs.p, nseg, cnt, out, keep);
    };
    uint64_t res[2] = {0, ~0ull};                                    // the batch's total, its lowest differing offset
    CJS_TRY(count_then_emit(s, nt, 2, count_scan, emit, diffs + std::min(n_diffs, cap), n_diffs < cap ? cap - n_diffs : 0, st, res));
    n_diffs += res[0]; first = std::min(first, res[1]); compared += P.bytes;
    return 0;
  }
};

void info_clear(cjs_bz_cmp_info* info) {
  memset(info, 0, sizeof *info);
  info->first_diff = info->first_bad_block = info->first_bad_block_b = ~0ull;
}

// cjs_bzip2_compare[_device]: the other side is plain bytes, one run
int compare_core(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const uint8_t* other, const uint8_t* d_other, size_t other_n,
                 uint64_t other_off, uint64_t off, uint64_t len, cjs_bz_diff* diffs, size_t cap, cjs_bz_cmp_info* info, const cjs_opts* opts) {
  clear_detail();
  if (!idx || !info || (!(other ? (const void*)other : (const void*)d_other) && other_n) || (!diffs && cap)) return CJS_E_INVALID_ARG;
  CJS_TRY(check_index_stream(in ? (const void*)in : (const void*)d_in, n, idx));
  info_clear(info);
  const uint64_t end = window_end(off, len, idx->off.back()), other_end = window_end(other_off, other_n, ~0ull);
  const uint64_t lo = std::max(off, other_off), hi = std::min(end, other_end);
  const std::vector<uint32_t> touched = blocks_under(idx->off, lo, hi);
  if (touched.empty()) return 0;
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  const int dev = cd.dev;
  if (d_in && (!on_device(d_in, dev) || !on_device(d_other, dev))) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  CompareCall C;
  const std::vector<CmRun> one(1, CmRun{other_off, other_end, (uint64_t)(uintptr_t)d_other});
  C.ix = idx; C.win_lo = lo; C.win_hi = hi; C.diffs = diffs; C.cap = cap;
  if (d_in) C.runs = &one;
  else { C.other = other; C.other_lo = other_off; C.other_hi = other_end; }
  RangeVerdicts V(idx);
  RangeStats st;
  CJS_TRY(range_engine(in, d_in, idx, touched, V, dev, st, [&](const RangeBatch& B) { return C.batch(B); }));
  info->n_diffs = C.n_diffs; info->first_diff = C.first; info->compared = C.compared; info->blocks_decoded = touched.size();
  const BadBlocks bad = V.bad_among(touched);
  info->n_bad_blocks = bad.n; info->first_bad_block = bad.first;
  if (bad.n) V.set_bad_detail(idx, (size_t)bad.first);
  if (env_debug())
    fprintf(stderr, "[cjs compare] %s: window [%llu, %llu), %zu of %zu blocks touched, %llu bad, %u passes (%u row batches, %u inverse-BWT batches), 1 windows, "
            "%llu tiles, other side uploaded %llu B, H2D %llu D2H %llu (of these the compare's own: H2D %llu D2H %llu), %llu diffs, %llu compared\n",
            d_in ? "device" : "host", (unsigned long long)lo, (unsigned long long)hi, touched.size(), idx->e.size(), (unsigned long long)bad.n, st.passes, st.a_batches,
            st.b_batches, (unsigned long long)C.st.tiles, (unsigned long long)C.other_up, (unsigned long long)(st.h2d + C.st.h2d), (unsigned long long)(st.d2h + C.st.d2h),
            (unsigned long long)C.st.h2d, (unsigned long long)C.st.d2h, (unsigned long long)C.n_diffs, (unsigned long long)C.compared);
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
  CJS_TRY(check_index_stream(a ? (const void*)a : (const void*)d_a, na, idx_a));
  CJS_TRY(check_index_stream(b ? (const void*)b : (const void*)d_b, nb, idx_b));
  info_clear(info);
  const bool device = !a;
  const uint64_t hi = window_end(off, len, std::min(idx_a->off.back(), idx_b->off.back()));
  if (off >= hi) return 0;
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  const int dev = cd.dev;
  if (device && (!on_device(d_a, dev) || !on_device(d_b, dev))) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  const uint64_t W = std::min(compare_window_bytes(), hi - off);
  DevBuf d_win((size_t)W + 64);
  if (!d_win.p) return CJS_E_OUT_OF_MEMORY;
  RangeVerdicts Va(idx_a), Vb(idx_b);
  CompareCall C;
  C.ix = idx_a; C.diffs = diffs; C.cap = cap;
  RangeStats st_a, st_b;
  uint32_t windows = 0;
  for (uint64_t wlo = off; wlo < hi; wlo += W, windows++) {
    const uint64_t whi = window_end(wlo, W, hi);
    // ---- B's window into the buffer: one range per touched block, so a bad block fails only its own range
    const std::vector<uint32_t> tb = blocks_under(idx_b->off, wlo, whi);
    std::vector<uint64_t> r_off, r_len, at;                          // (at: where block k's first byte would stand: byte o of the window at d_win + (o - wlo))
    for (uint32_t k : tb) {
      const uint64_t lo = std::max(idx_b->off[k], wlo), e = std::min(idx_b->off[k + 1], whi);
      r_off.push_back(lo); r_len.push_back(e - lo); at.push_back((uint64_t)(uintptr_t)d_win.p + (idx_b->off[k] - wlo));
    }
    CJS_TRY(range_read_to_device(b, d_b, idx_b, r_off.data(), r_len.data(), r_off.size(), (uint8_t*)d_win.p, Vb, dev, st_b));
    const std::vector<CmRun> runs = good_runs(tb.data(), at.data(), tb.size(), Vb.verdict, idx_b->off, wlo, whi);      // the good ranges, neighbours merged
    // ---- A's blocks of the window against those runs (B's read has returned: the engine is not re-entered)
    C.win_lo = wlo; C.win_hi = whi; C.runs = &runs;
    CJS_TRY(range_engine(a, d_a, idx_a, blocks_under(idx_a->off, wlo, whi), Va, dev, st_a, [&](const RangeBatch& B) { return C.batch(B); }));
  }
  const std::vector<uint32_t> ta = blocks_under(idx_a->off, off, hi), tb = blocks_under(idx_b->off, off, hi);
  info->n_diffs = C.n_diffs; info->first_diff = C.first; info->compared = C.compared; info->blocks_decoded = ta.size();
  const BadBlocks bad_a = Va.bad_among(ta), bad_b = Vb.bad_among(tb);
  info->n_bad_blocks = bad_a.n; info->first_bad_block = bad_a.first;
  info->n_bad_blocks_b = bad_b.n; info->first_bad_block_b = bad_b.first;
  if (bad_a.n) Va.set_bad_detail(idx_a, (size_t)bad_a.first);
  else if (bad_b.n) Vb.set_bad_detail(idx_b, (size_t)bad_b.first);
  if (env_debug())
    fprintf(stderr, "[cjs compare] %s streams: window [%llu, %llu), %zu of %zu blocks touched, %llu bad, %u passes (%u row batches, %u inverse-BWT batches), %u windows "
            "of %llu B (other stream: %zu of %zu blocks, %llu bad, %u passes), %llu tiles, other side uploaded 0 B, H2D %llu D2H %llu (of these the compare's own: "
            "H2D %llu D2H %llu), %llu diffs, %llu compared\n",
            device ? "device" : "host", (unsigned long long)off, (unsigned long long)hi, ta.size(), idx_a->e.size(), (unsigned long long)bad_a.n, st_a.passes,
            st_a.a_batches, st_a.b_batches, windows, (unsigned long long)W, tb.size(), idx_b->e.size(), (unsigned long long)bad_b.n, st_b.passes,
            (unsigned long long)C.st.tiles, (unsigned long long)(st_a.h2d + st_b.h2d + C.st.h2d), (unsigned long long)(st_a.d2h + st_b.d2h + C.st.d2h),
            (unsigned long long)C.st.h2d, (unsigned long long)C.st.d2h, (unsigned long long)C.n_diffs, (unsigned long long)C.compared);
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
