// regex.hip -- bounded regular-expression search in a .bz2 stream (cjs_bzip2_search_regex[_device]): the literal
// search (search.hip) with another match function.  No automaton state is carried from byte to byte: every start position is
// judged on its own, by walking its patterns' tables (rx_compile.h) over at most 256 bytes in front of it, so the segments, the
// carry, the tiles with their halo (scan_text.h), sr_scan and the count-then-emit round are the literal search's.
//   rx_count   per 16 KiB tile of a segment: the number of matches that start in it
//   rx_emit    the matches of a tile again, with their lengths, written at base + rank
#include "scan_text.h"
#include "rx_compile.h"
#include <string.h>

using namespace cjs;

namespace cjs {

__global__ void sr_scan(uint64_t* __restrict__ cnt, uint64_t nt);      // (search.hip)

struct RxLds {
  alignas(16) uint32_t text[SR_TEXT / 4];
  alignas(16) uint32_t blob[RX_MAX_BLOB / 4];      // the compiled patterns (rx_compile.h: header, class map, first[], tables)
  uint32_t row[SR_ROWS];
  uint32_t scan[4];
};
static_assert(sizeof(RxLds) < 64 * 1024 && 3 * sizeof(RxLds) <= 160 * 1024, "static LDS; three workgroups to a CU");
static_assert(SR_TEXT % 16 == 0 && RX_MAX_BLOB % 16 == 0, "both are copied as 16-byte vectors");

// Tile blockIdx.x: the blob (nvec vectors of 16 bytes) and the tile's text into LDS.
__device__ __forceinline__ SrTile rx_stage(RxLds& L, const SrSeg* __restrict__ segs, uint32_t nseg, const uint4* __restrict__ blob, uint32_t nvec, uint32_t maxlen,
                                           const uint8_t* __restrict__ carry, uint32_t fold) {
  for (uint32_t v = threadIdx.x; v < nvec; v += 256) reinterpret_cast<uint4*>(L.blob)[v] = blob[v];
  return sr_stage_text(L.text, segs, nseg, maxlen, carry, fold);
}

// The patterns that match at position i of the tile, as a mask.  first[] of the position's byte names the patterns whose start
// state survives it; each of those is walked from its start state over at most min(maxlen, room) bytes (rx_walk: the last
// accepting step is the match's length).  Position, window and room are sr_match's.
__device__ __forceinline__ uint64_t rx_match(const RxLds& L, const SrTile& T, uint32_t maxlen, uint32_t i, uint64_t win_lo, uint64_t win_hi) {
  const uint64_t o = T.off0 + i;
  if (i >= T.npos || o < win_lo || o >= win_hi) return 0;
  const uint32_t room = (uint32_t)min(min(T.left - i, win_hi - o), (uint64_t)maxlen);
  const uint8_t* t = reinterpret_cast<const uint8_t*>(L.text) + T.sh + i;
  const uint8_t* B = reinterpret_cast<const uint8_t*>(L.blob);
  uint64_t m = 0;
  for (uint64_t f = rx_first(B, t[0]); f; f &= f - 1) {
    const uint32_t j = (uint32_t)__builtin_ctzll(f);
    if (rx_walk(B, j, t, room)) m |= 1ull << j;
  }
  return m;
}

__global__ __launch_bounds__(256) void rx_count(const SrSeg* __restrict__ segs, uint32_t nseg, const uint4* __restrict__ blob, uint32_t nvec, uint32_t maxlen,
                                                const uint8_t* __restrict__ carry, uint32_t fold, uint64_t win_lo, uint64_t win_hi, uint64_t* __restrict__ cnt) {
  __shared__ RxLds L;
  const SrTile T = rx_stage(L, segs, nseg, blob, nvec, maxlen, carry, fold);
  uint32_t c = 0;
  for (uint32_t r = wave_id(); r * 64 < T.npos; r += 4) c += (uint32_t)__popcll(rx_match(L, T, maxlen, r * 64 + lane_id(), win_lo, win_hi));
  const uint32_t total = block_sum<256, uint32_t>(c, L.scan);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// Match number `rank` of the batch (ranks ascend with the tile, the row, the lane and the pattern: sorted by (off, pattern)) goes to
// out[rank] if it is among the first `keep`; sr_emit's ranks, no atomics.
__global__ __launch_bounds__(256) void rx_emit(const SrSeg* __restrict__ segs, uint32_t nseg, const uint4* __restrict__ blob, uint32_t nvec, uint32_t maxlen,
                                               const uint8_t* __restrict__ carry, uint32_t fold, uint64_t win_lo, uint64_t win_hi, const uint64_t* __restrict__ cnt,
                                               uint4* __restrict__ out, uint64_t keep) {
  __shared__ RxLds L;
  const uint64_t base = cnt[blockIdx.x];
  if (cnt[blockIdx.x + 1] == base || base >= keep) return;
  L.row[threadIdx.x] = 0;
  const SrTile T = rx_stage(L, segs, nseg, blob, nvec, maxlen, carry, fold);
  for (uint32_t r = wave_id(); r * 64 < T.npos; r += 4) {
    const uint32_t s = wave_sum((uint32_t)__popcll(rx_match(L, T, maxlen, r * 64 + lane_id(), win_lo, win_hi)));
    if (lane_id() == 0) L.row[r] = s;
  }
  __syncthreads();
  uint32_t tot;
  const uint32_t ex = block_excl_sum<256, uint32_t>(L.row[threadIdx.x], L.scan, tot);
  L.row[threadIdx.x] = ex;
  __syncthreads();
  for (uint32_t r = wave_id(); r * 64 < T.npos; r += 4) {
    if ((r + 1 < SR_ROWS ? L.row[r + 1] : tot) == L.row[r]) continue;      // a row without a match: nothing to recompute
    const uint32_t i = r * 64 + lane_id();
    const uint64_t o = T.off0 + i;
    // the lane's mask first (its rank needs the whole wave's counts), then only the patterns of the mask again, for their lengths
    uint64_t m = rx_match(L, T, maxlen, i, win_lo, win_hi);
    const uint32_t c = (uint32_t)__popcll(m);
    uint64_t rank = base + L.row[r] + (wave_incl_sum(c) - c);
    if (!m) continue;
    const uint32_t room = (uint32_t)min(min(T.left - i, win_hi - o), (uint64_t)maxlen);
    const uint8_t* t = reinterpret_cast<const uint8_t*>(L.text) + T.sh + i;
    for (; m && rank < keep; m &= m - 1, rank++) {
      const uint32_t j = (uint32_t)__builtin_ctzll(m);
      out[rank] = make_uint4((uint32_t)o, (uint32_t)(o >> 32), j, rx_walk(reinterpret_cast<const uint8_t*>(L.blob), j, t, room));
    }
  }
}

}  // namespace cjs

// ---------------------------------------------------------------- the driver
namespace {

// One call: the blob on the device, the carry (two buffers, written in turn: a batch reads the one the batch before wrote), the
// list so far.  The shape of search.hip's SearchCall.
struct RegexCall {
  const cjs_bz_index* ix = nullptr;
  RxProgram prog;
  uint32_t fold = 0;
  uint64_t win_lo = 0, win_hi = 0;
  cjs_bz_match* found = nullptr; uint64_t cap = 0, n_matches = 0;
  Owner<void*, PoolGive> mem;                                                 // the blob, then the two carry buffers of SR_MAXL bytes
  int cur = 0; SearchCarry held;                                   // the carry's bytes stand in buffer `cur`
  ScanStats st;
  uint8_t* carry(int k) const { return (uint8_t*)mem.p + prog.blob.size() + SR_MAXL * (size_t)k; }

  int device_state() {                                             // (at the first batch: the device is current then)
    if (mem.p) return 0;
    mem = DevBuf(prog.blob.size() + 2 * SR_MAXL);
    if (!mem.p) return CJS_E_OUT_OF_MEMORY;
    if (hipMemcpy(mem.p, prog.blob.data(), prog.blob.size(), hipMemcpyHostToDevice) != hipSuccess) return CJS_E_HIP;
    st.h2d += prog.blob.size();
    return 0;
  }

  // The matches of `segs` (npos set, in order), appended to the list.  Returns with the stream drained.
  int scan_segments(hipStream_t s, std::vector<SearchSeg>& segs) {
    const uint64_t nt = tile_segments(segs, SR_TILE);
    const uint4* d_blob = (const uint4*)mem.p;
    const uint32_t nseg = (uint32_t)segs.size(), nvec = (uint32_t)(prog.blob.size() / 16), maxlen = prog.maxlen;
    Owner<void*, PoolGive> d_segs;
    auto count_scan = [&](uint64_t* cnt) {
      d_segs = DevBuf(sizeof(SearchSeg) * segs.size());
      if (!d_segs.p) return (int)CJS_E_OUT_OF_MEMORY;
      if (hipMemcpyAsync(d_segs.p, segs.data(), sizeof(SearchSeg) * segs.size(), hipMemcpyHostToDevice, s) != hipSuccess) return (int)CJS_E_HIP;
      st.h2d += sizeof(SearchSeg) * segs.size();
      hipLaunchKernelGGL(rx_count, dim3((unsigned)nt), dim3(256), 0, s, (const SrSeg*)d_segs.p, nseg, d_blob, nvec, maxlen, (const uint8_t*)carry(cur), fold, win_lo, win_hi, cnt);
      hipLaunchKernelGGL(sr_scan, dim3(1), dim3(256), 0, s, cnt, nt);
      return 0;
    };
    auto emit = [&](const uint64_t* cnt, uint4* out, uint64_t keep) {
      hipLaunchKernelGGL(rx_emit, dim3((unsigned)nt), dim3(256), 0, s, (const SrSeg*)d_segs.p, nseg, d_blob, nvec, maxlen, (const uint8_t*)carry(cur), fold, win_lo, win_hi, cnt, out,
                         keep);
    };
    uint64_t total = 0;
    CJS_TRY(count_then_emit(s, nt, 1, count_scan, emit, found + std::min(n_matches, cap), n_matches < cap ? cap - n_matches : 0, st, &total));
    n_matches += total;
    return 0;
  }

  // A decoded batch: its segments and the new carry (search_plan, with the longest possible match in the longest pattern's place)
  int batch(const RangeBatch& B) {
    if (const int rc = device_state()) return drained(B.s, rc);
    SearchPlan P = search_plan(B.good_runs(ix->off, 0, ~0ull), held, prog.maxlen);
    if (P.segs.empty()) return 0;                                    // no good block: the carry waits on
    const SearchSeg& last = P.segs.back();
    uint8_t* to = carry(cur ^ 1);                                    // the last P.hold bytes of the prefix and the segment
    int rc = 0;
    if (P.from_pre && hipMemcpyAsync(to, carry(cur) + (last.pre - P.from_pre), (size_t)P.from_pre, hipMemcpyDeviceToDevice, B.s) != hipSuccess) rc = CJS_E_HIP;
    const uint64_t from_seg = P.hold - P.from_pre;
    if (!rc && from_seg && hipMemcpyAsync(to + P.from_pre, (const uint8_t*)(uintptr_t)last.src + (last.len - from_seg), (size_t)from_seg, hipMemcpyDeviceToDevice, B.s) != hipSuccess)
      rc = CJS_E_HIP;
    const int rc2 = scan_segments(B.s, P.segs);
    if (rc || rc2) return rc ? rc : rc2;
    cur ^= P.hold ? 1 : 0; held = P.next;
    return 0;
  }

  int finish() {                                                     // what still waits in the carry
    if (!held.len) return 0;
    Stream s;
    if (hipStreamCreate(s.put()) != hipSuccess) return CJS_E_HIP;
    std::vector<SearchSeg> segs(1, carry_segment(held));
    const int rc = scan_segments(s, segs);
    held.len = 0;
    return rc;
  }
};

// the argument errors of cjs_bzip2_search, then the compiler's refusals (rx_compile checks the pattern count, the flags and pat_off)
int regex_check_args(const void* in, size_t n, const cjs_bz_index* idx, const uint8_t* pat, const uint32_t* pat_off, uint32_t npat, uint32_t flags,
                     const cjs_bz_match* found, size_t cap, const cjs_bz_search_info* info, RxProgram& prog) {
  if (!idx || !info || !pat || !pat_off || (!in && n) || (!found && cap)) return CJS_E_INVALID_ARG;
  CJS_TRY(check_index_stream(in, n, idx));
  RxError err;
  const int rc = rx_compile(pat, pat_off, npat, flags, prog, err);
  if (rc) set_detail("%s", err.text);
  return rc;
}

int regex_core(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const uint8_t* pat, const uint32_t* pat_off, uint32_t npat,
               uint32_t flags, uint64_t off, uint64_t len, cjs_bz_match* found, size_t cap, cjs_bz_search_info* info, const cjs_opts* opts) {
  clear_detail();
  RegexCall C;
  CJS_TRY(regex_check_args(in ? (const void*)in : (const void*)d_in, n, idx, pat, pat_off, npat, flags, found, cap, info, C.prog));
  info->n_matches = info->n_bad_blocks = info->blocks_decoded = 0; info->first_bad_block = ~0ull;
  const uint64_t win_hi = window_end(off, len, idx->off.back());
  const std::vector<uint32_t> touched = blocks_under(idx->off, off, win_hi);
  if (touched.empty()) return 0;
  CallDevice cd;
  CJS_TRY(cd.select(opts));
  if (d_in && !on_device(d_in, cd.dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  C.ix = idx; C.fold = flags & CJS_SEARCH_NOCASE; C.win_lo = off; C.win_hi = win_hi; C.found = found; C.cap = cap;
  RangeVerdicts V(idx);
  RangeStats st;
  CJS_TRY(range_engine(in, d_in, idx, touched, V, cd.dev, st, [&](const RangeBatch& B) { return C.batch(B); }));
  CJS_TRY(C.finish());
  info->n_matches = C.n_matches; info->blocks_decoded = touched.size();
  const BadBlocks bad = V.bad_among(touched);
  info->n_bad_blocks = bad.n; info->first_bad_block = bad.first;
  if (bad.n) V.set_bad_detail(idx, (size_t)bad.first);
  if (env_debug()) {
    const RxHeader* H = (const RxHeader*)C.prog.blob.data();
    fprintf(stderr, "[cjs regex] %s: %u patterns (%u classes, tables %u B, longest match %u), window [%llu, %llu), %zu of %zu blocks touched, %llu bad, %u passes (%u row batches, "
            "%u inverse-BWT batches), upload %llu B, %llu tiles, H2D %llu D2H %llu, %llu matches\n", d_in ? "device" : "host", npat, H->nclass, H->nbytes, C.prog.maxlen,
            (unsigned long long)off, (unsigned long long)win_hi, touched.size(), idx->e.size(), (unsigned long long)info->n_bad_blocks, st.passes, st.a_batches, st.b_batches,
            (unsigned long long)st.up, (unsigned long long)C.st.tiles, (unsigned long long)(st.h2d + C.st.h2d), (unsigned long long)(st.d2h + C.st.d2h),
            (unsigned long long)C.n_matches);
  }
  return 0;
}

}  // namespace

extern "C" int cjs_bzip2_search_regex(const uint8_t* in, size_t n, const cjs_bz_index* idx, const uint8_t* pat, const uint32_t* pat_off, uint32_t npat, uint32_t flags,
                                      uint64_t off, uint64_t len, cjs_bz_match* found, size_t cap, cjs_bz_search_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  return regex_core(in, nullptr, n, idx, pat, pat_off, npat, flags, off, len, found, cap, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_search_regex_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const uint8_t* pat, const uint32_t* pat_off, uint32_t npat,
                                             uint32_t flags, uint64_t off, uint64_t len, cjs_bz_match* found, size_t cap, cjs_bz_search_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  return regex_core(nullptr, d_in, n, idx, pat, pat_off, npat, flags, off, len, found, cap, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_regex_check(const uint8_t* pat, const uint32_t* pat_off, uint32_t npat, uint32_t flags, uint32_t* states, uint32_t* max_len) {
  CJS_GUARD_BEGIN
  clear_detail();
  if (!pat || !pat_off) return CJS_E_INVALID_ARG;
  RxProgram prog; RxError err;
  const int rc = rx_compile(pat, pat_off, npat, flags, prog, err);
  if (rc) { set_detail("%s", err.text); return rc; }
  for (uint32_t j = 0; j < npat; j++) { if (states) states[j] = prog.states[j]; if (max_len) max_len[j] = prog.max_len[j]; }
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_stage_regex_scan(const uint8_t* pat, const uint32_t* pat_off, uint32_t npat, uint32_t flags, const uint8_t* text, size_t n, cjs_bz_match* found,
                                    size_t cap, size_t* n_found) {
  CJS_GUARD_BEGIN
  clear_detail();
  if (!pat || !pat_off || !n_found || (!text && n) || (!found && cap)) return CJS_E_INVALID_ARG;
  RxProgram prog; RxError err;
  const int rc = rx_compile(pat, pat_off, npat, flags, prog, err);
  if (rc) { set_detail("%s", err.text); return rc; }
  size_t k = 0;
  rx_scan(prog, text, n, [&](uint64_t o, uint32_t j, uint32_t len) { if (k < cap) found[k] = cjs_bz_match{o, j, len}; k++; });
  *n_found = k;
  return 0;
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
