// search.hip -- pattern search in a .bz2 stream (cjs_bzip2_search[_device]): the second consumer of the pass engine
// of the indexed entry points (range_engine.h).  Every decoded inverse-BWT batch is scanned where it stands expanded in device
// scratch; 16 bytes per match leave the GPU.
//   sr_count   per 16 KiB tile of a segment: the number of matches that start in it
//   sr_scan    the exclusive scan of the tile counts (one workgroup), the batch's total behind them
//   sr_emit    the matches of a tile again, written at base + rank
// A segment is a run of GOOD, index-consecutive blocks of a batch, possibly with a prefix from the call's carry buffer: the last
// (longest pattern - 1) bytes of the batch before, where a match that ends in this batch may start (search_plan of scan_plan.h).
#include "scan_text.h"
#include <string.h>

using namespace cjs;

namespace cjs {

struct SrPatTab {          // the patterns as the kernels read them (folded under NOCASE)
  uint32_t npat, maxlen, nbytes, pad;
  uint32_t word[SR_MAXP], mask[SR_MAXP];      // the first up-to-4 bytes, little-endian, and the mask of those that exist
  uint32_t plen[SR_MAXP], poff[SR_MAXP];
  uint8_t bytes[SR_MAXP * SR_MAXL];
};
struct SrLds {
  uint32_t text[SR_TEXT / 4];
  uint32_t word[SR_MAXP], mask[SR_MAXP], plen[SR_MAXP], poff[SR_MAXP];
  uint32_t pat[SR_MAXP * SR_MAXL / 4];
  uint32_t row[SR_ROWS];
  uint32_t scan[4];
};

// Tile blockIdx.x: the patterns and the tile's bytes (+ the halo) into LDS (the text: sr_stage_text of scan_text.h).
__device__ __forceinline__ SrTile sr_stage(SrLds& L, const SrSeg* __restrict__ segs, uint32_t nseg, const SrPatTab* __restrict__ tab,
                                           const uint8_t* __restrict__ carry, uint32_t fold) {
  const uint32_t npat = tab->npat;
  if (threadIdx.x < npat) {
    L.word[threadIdx.x] = tab->word[threadIdx.x]; L.mask[threadIdx.x] = tab->mask[threadIdx.x];
    L.plen[threadIdx.x] = tab->plen[threadIdx.x]; L.poff[threadIdx.x] = tab->poff[threadIdx.x];
  }
  for (uint32_t v = threadIdx.x; v < (tab->nbytes + 15) / 16; v += 256) reinterpret_cast<uint4*>(L.pat)[v] = reinterpret_cast<const uint4*>(tab->bytes)[v];
  SrTile T = sr_stage_text(L.text, segs, nseg, tab->maxlen, carry, fold);
  T.npat = npat;
  return T;
}

// The patterns that match at position i of the tile, as a mask.  One masked compare of the first four bytes rejects a pattern; the
// rest is verified only then.  A match lies inside the window and inside the segment's bytes.
__device__ __forceinline__ uint64_t sr_match(const SrLds& L, const SrTile& T, uint32_t i, uint64_t win_lo, uint64_t win_hi) {
  const uint64_t o = T.off0 + i;
  if (i >= T.npos || o < win_lo || o >= win_hi) return 0;
  const uint64_t room = min(T.left - i, win_hi - o);
  const uint32_t li = T.sh + i;
  const uint32_t w = __builtin_amdgcn_alignbyte(L.text[(li >> 2) + 1], L.text[li >> 2], li & 3u);
  const uint8_t* t = reinterpret_cast<const uint8_t*>(L.text) + li;
  uint64_t m = 0;
  for (uint32_t j = 0; j < T.npat; j++) {
    if ((w ^ L.word[j]) & L.mask[j]) continue;
    const uint32_t pl = L.plen[j];
    if (pl > room) continue;
    const uint8_t* p = reinterpret_cast<const uint8_t*>(L.pat) + L.poff[j];
    uint32_t k = 4;
    while (k < pl && t[k] == p[k]) k++;
    if (k >= pl) m |= 1ull << j;
  }
  return m;
}

__global__ __launch_bounds__(256) void sr_count(const SrSeg* __restrict__ segs, uint32_t nseg, const SrPatTab* __restrict__ tab, const uint8_t* __restrict__ carry,
                                                uint32_t fold, uint64_t win_lo, uint64_t win_hi, uint64_t* __restrict__ cnt) {
  __shared__ SrLds L;
  const SrTile T = sr_stage(L, segs, nseg, tab, carry, fold);
  uint32_t c = 0;
  for (uint32_t r = wave_id(); r * 64 < T.npos; r += 4) c += (uint32_t)__popcll(sr_match(L, T, r * 64 + lane_id(), win_lo, win_hi));
  const uint32_t total = block_sum<256, uint32_t>(c, L.scan);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// cnt[0 .. nt) -> their exclusive prefix sums, cnt[nt] = the total
__global__ __launch_bounds__(256) void sr_scan(uint64_t* __restrict__ cnt, uint64_t nt) {
  __shared__ uint64_t sm[4];
  const uint64_t run = rg_scan_counts(cnt, nt, sm, [](uint64_t) {});
  if (threadIdx.x == 0) cnt[nt] = run;
}

// Match number `rank` of the batch (ranks ascend with the tile, the row, the lane and the pattern: sorted by (off, pattern)) goes to
// out[rank] if it is among the first `keep`.  No atomics: the ranks come from the scan, the row counts and the wave's prefix sums.
__global__ __launch_bounds__(256) void sr_emit(const SrSeg* __restrict__ segs, uint32_t nseg, const SrPatTab* __restrict__ tab, const uint8_t* __restrict__ carry,
                                               uint32_t fold, uint64_t win_lo, uint64_t win_hi, const uint64_t* __restrict__ cnt, uint4* __restrict__ out, uint64_t keep) {
  __shared__ SrLds L;
  const uint64_t base = cnt[blockIdx.x];
  if (cnt[blockIdx.x + 1] == base || base >= keep) return;
  L.row[threadIdx.x] = 0;
  const SrTile T = sr_stage(L, segs, nseg, tab, carry, fold);
  for (uint32_t r = wave_id(); r * 64 < T.npos; r += 4) {
    const uint32_t s = wave_sum((uint32_t)__popcll(sr_match(L, T, r * 64 + lane_id(), win_lo, win_hi)));
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
    uint64_t m = sr_match(L, T, i, win_lo, win_hi);
    const uint32_t c = (uint32_t)__popcll(m);
    uint64_t rank = base + L.row[r] + (wave_incl_sum(c) - c);
    const uint64_t o = T.off0 + i;
    for (; m && rank < keep; m &= m - 1, rank++) out[rank] = make_uint4((uint32_t)o, (uint32_t)(o >> 32), (uint32_t)__builtin_ctzll(m), 0u);
  }
}

}  // namespace cjs

// ---------------------------------------------------------------- the driver
namespace {

// One call: the patterns on the device, the carry (two buffers, written in turn: a batch reads the one the batch before wrote),
// the list so far.
struct SearchCall {
  const cjs_bz_index* ix = nullptr;
  SrPatTab tab;
  uint32_t fold = 0;
  uint64_t win_lo = 0, win_hi = 0;
  cjs_bz_match* found = nullptr; uint64_t cap = 0, n_matches = 0;
  Owner<void*, PoolGive> mem;                                                 // SrPatTab, then the two carry buffers of SR_MAXL bytes
  int cur = 0; SearchCarry held;                                   // the carry's bytes stand in buffer `cur`
  ScanStats st;
  uint8_t* carry(int k) const { return (uint8_t*)mem.p + sizeof(SrPatTab) + SR_MAXL * (size_t)k; }

  int device_state() {                                             // (at the first batch: the device is current then)
    if (mem.p) return 0;
    mem = DevBuf(sizeof(SrPatTab) + 2 * SR_MAXL);
    if (!mem.p) return CJS_E_OUT_OF_MEMORY;
    if (hipMemcpy(mem.p, &tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) return CJS_E_HIP;
    st.h2d += sizeof tab;
    return 0;
  }

  // The matches of `segs` (npos set, in order), appended to the list.  Returns with the stream drained.
  int scan_segments(hipStream_t s, std::vector<SearchSeg>& segs) {
    const uint64_t nt = tile_segments(segs, SR_TILE);
    const SrPatTab* d_tab = (const SrPatTab*)mem.p;
    const uint32_t nseg = (uint32_t)segs.size();
    Owner<void*, PoolGive> d_segs;
    auto count_scan = [&](uint64_t* cnt) {
      d_segs = DevBuf(sizeof(SearchSeg) * segs.size());
      if (!d_segs.p) return (int)CJS_E_OUT_OF_MEMORY;
      if (hipMemcpyAsync(d_segs.p, segs.data(), sizeof(SearchSeg) * segs.size(), hipMemcpyHostToDevice, s) != hipSuccess) return (int)CJS_E_HIP;
      st.h2d += sizeof(SearchSeg) * segs.size();
      hipLaunchKernelGGL(sr_count, dim3((unsigned)nt), dim3(256), 0, s, (const SrSeg*)d_segs.p, nseg, d_tab, (const uint8_t*)carry(cur), fold, win_lo, win_hi, cnt);
      hipLaunchKernelGGL(sr_scan, dim3(1), dim3(256), 0, s, cnt, nt);
      return 0;
    };
    auto emit = [&](const uint64_t* cnt, uint4* out, uint64_t keep) {
      hipLaunchKernelGGL(sr_emit, dim3((unsigned)nt), dim3(256), 0, s, (const SrSeg*)d_segs.p, nseg, d_tab, (const uint8_t*)carry(cur), fold, win_lo, win_hi, cnt, out, keep);
    };
    uint64_t total = 0;
    CJS_TRY(count_then_emit(s, nt, 1, count_scan, emit, found + std::min(n_matches, cap), n_matches < cap ? cap - n_matches : 0, st, &total));
    n_matches += total;
    return 0;
  }

  // A decoded batch: its segments and the new carry (search_plan); the last segment's tail is tested with the next batch (or by
  // finish()).
  int batch(const RangeBatch& B) {
    if (const int rc = device_state()) return drained(B.s, rc);
    SearchPlan P = search_plan(B.good_runs(ix->off, 0, ~0ull), held, tab.maxlen);
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

int search_check_args(const void* in, size_t n, const cjs_bz_index* idx, const uint8_t* pat, const uint32_t* pat_off, uint32_t npat, uint32_t flags,
                      const cjs_bz_match* found, size_t cap, const cjs_bz_search_info* info, SrPatTab& tab) {
  if (!idx || !info || !pat || !pat_off || (!in && n) || (!found && cap)) return CJS_E_INVALID_ARG;
  CJS_TRY(check_index_stream(in, n, idx));
  if (npat < 1 || npat > SR_MAXP) { set_detail("1 to %u patterns", SR_MAXP); return CJS_E_INVALID_ARG; }
  if (flags & ~(uint32_t)CJS_SEARCH_NOCASE) { set_detail("undefined flag bits"); return CJS_E_INVALID_ARG; }
  if (pat_off[0] != 0) { set_detail("pat_off[0] is not 0"); return CJS_E_INVALID_ARG; }
  memset(&tab, 0, sizeof tab);
  tab.npat = npat;
  for (uint32_t j = 0; j < npat; j++) {
    const uint32_t pl = pat_off[j + 1] - pat_off[j];
    if (pat_off[j + 1] < pat_off[j] || pl < 1 || pl > SR_MAXL) { set_detail("pattern %u: a length outside 1..%u", j, SR_MAXL); return CJS_E_INVALID_ARG; }
    tab.plen[j] = pl; tab.poff[j] = pat_off[j];
    tab.maxlen = std::max(tab.maxlen, pl);
    for (uint32_t k = 0; k < pl; k++) {
      uint8_t c = pat[pat_off[j] + k];
      if ((flags & CJS_SEARCH_NOCASE) && c >= 'A' && c <= 'Z') c += 32;
      tab.bytes[pat_off[j] + k] = c;
      if (k < 4) { tab.word[j] |= (uint32_t)c << (8 * k); tab.mask[j] |= 0xFFu << (8 * k); }
    }
  }
  tab.nbytes = pat_off[npat];
  return 0;
}

int search_core(const uint8_t* in, const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const uint8_t* pat, const uint32_t* pat_off, uint32_t npat,
                uint32_t flags, uint64_t off, uint64_t len, cjs_bz_match* found, size_t cap, cjs_bz_search_info* info, const cjs_opts* opts) {
  clear_detail();
  SearchCall C;
  CJS_TRY(search_check_args(in ? (const void*)in : (const void*)d_in, n, idx, pat, pat_off, npat, flags, found, cap, info, C.tab));
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
  if (env_debug())
    fprintf(stderr, "[cjs search] %s: %u patterns (longest %u), window [%llu, %llu), %zu of %zu blocks touched, %llu bad, %u passes (%u row batches, %u inverse-BWT batches), "
            "upload %llu B, %llu tiles, H2D %llu D2H %llu, %llu matches\n", d_in ? "device" : "host", npat, C.tab.maxlen, (unsigned long long)off, (unsigned long long)win_hi,
            touched.size(), idx->e.size(), (unsigned long long)info->n_bad_blocks, st.passes, st.a_batches, st.b_batches, (unsigned long long)st.up,
            (unsigned long long)C.st.tiles, (unsigned long long)(st.h2d + C.st.h2d), (unsigned long long)(st.d2h + C.st.d2h), (unsigned long long)C.n_matches);
  return 0;
}

}  // namespace

extern "C" int cjs_bzip2_search(const uint8_t* in, size_t n, const cjs_bz_index* idx, const uint8_t* pat, const uint32_t* pat_off, uint32_t npat, uint32_t flags,
                                uint64_t off, uint64_t len, cjs_bz_match* found, size_t cap, cjs_bz_search_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  return search_core(in, nullptr, n, idx, pat, pat_off, npat, flags, off, len, found, cap, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}

extern "C" int cjs_bzip2_search_device(const uint8_t* d_in, size_t n, const cjs_bz_index* idx, const uint8_t* pat, const uint32_t* pat_off, uint32_t npat,
                                       uint32_t flags, uint64_t off, uint64_t len, cjs_bz_match* found, size_t cap, cjs_bz_search_info* info, const cjs_opts* opts) {
  CJS_GUARD_BEGIN
  return search_core(nullptr, d_in, n, idx, pat, pat_off, npat, flags, off, len, found, cap, info, opts);
  CJS_GUARD_END(CJS_E_OUT_OF_MEMORY, CJS_E_HIP)
}
