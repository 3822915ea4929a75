// search.hip -- pattern search in a .bz2 stream (cjs_bzip2_search[_device]): the second consumer of the pass engine
// of the indexed entry points (range_engine.h).  Every decoded inverse-BWT batch is scanned where it stands expanded in device
// scratch; 16 bytes per match leave the GPU.
//   sr_count   per 16 KiB tile of a segment: the number of matches that start in it
//   sr_scan    the exclusive scan of the tile counts (one workgroup), the batch's total behind them
//   sr_emit    the matches of a tile again, written at base + rank
// A segment is a run of GOOD, index-consecutive blocks of a batch, possibly with a prefix from the call's carry buffer: the last
// (longest pattern - 1) bytes of the batch before, where a match that ends in this batch may start.
#include "range_engine.h"
#include "prims.hpp"
#include <string.h>

using namespace cjs;

namespace cjs {

constexpr uint32_t SR_TILE = 16384;                                        // start positions of a tile (a power of two >= 1024)
constexpr uint32_t SR_ROWS = SR_TILE / 64;                                 // a row = the 64 positions a wave tests at once
constexpr uint32_t SR_MAXP = CJS_SEARCH_MAX_PATTERNS, SR_MAXL = CJS_SEARCH_MAX_PATTERN_BYTES;
constexpr uint32_t SR_TEXT = (15 + SR_TILE + SR_MAXL - 1 + 15) / 16 * 16 + 16;      // staged bytes at any alignment, + the word behind the last
static_assert(SR_ROWS == 256 && SR_MAXP == 64, "one row per thread of the block scan, one mask bit per pattern");

struct SrSeg {
  uint64_t src, len;       // len bytes at device address src ...
  uint64_t off;            // ... behind `pre` bytes of the carry buffer; decoded offset of the first of all these bytes
  uint64_t npos;           // start positions tested: [0, npos) of the pre + len bytes
  uint64_t tile0;          // the segment's first tile
  uint32_t pre, pad;
};
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
struct SrTile { uint64_t off0, left; uint32_t npos, sh, npat; };      // decoded offset of and bytes from position 0; positions; its LDS byte

// 'A'..'Z' -> 'a'..'z' in the four bytes of w
__device__ __forceinline__ uint32_t sr_fold4(uint32_t w) {
  const uint32_t h = w & 0x7F7F7F7Fu;
  const uint32_t m = (h + 0x3F3F3F3Fu) & ~(h + 0x25252525u) & ~w & 0x80808080u;      // bit 7: 0x41 <= byte <= 0x5A
  return w | (m >> 2);
}

// Tile blockIdx.x: its segment, the patterns and the tile's bytes (+ the halo) into LDS.  Byte i of the tile is at LDS byte sh + i,
// congruent mod 16 to its device address, so the loads are aligned vectors bounded to the segment (rg_ld16).
__device__ __forceinline__ SrTile sr_stage(SrLds& L, const SrSeg* __restrict__ segs, uint32_t nseg, const SrPatTab* __restrict__ tab,
                                           const uint8_t* __restrict__ carry, uint32_t fold) {
  const uint64_t t = blockIdx.x;
  uint32_t lo = 0, hi = nseg;                                                // the last segment with tile0 <= t
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (segs[mid].tile0 <= t) lo = mid; else hi = mid; }
  const SrSeg g = segs[lo];
  const uint32_t npat = tab->npat, maxlen = tab->maxlen;
  const uint64_t p0 = (t - g.tile0) * SR_TILE, n = g.pre + g.len;
  SrTile T;
  T.npos = (uint32_t)min((uint64_t)SR_TILE, g.npos - p0);
  T.left = n - p0; T.off0 = g.off + p0; T.npat = npat;
  const uint32_t nbytes = (uint32_t)min(T.left, (uint64_t)(T.npos + maxlen - 1));
  if (threadIdx.x < npat) {
    L.word[threadIdx.x] = tab->word[threadIdx.x]; L.mask[threadIdx.x] = tab->mask[threadIdx.x];
    L.plen[threadIdx.x] = tab->plen[threadIdx.x]; L.poff[threadIdx.x] = tab->poff[threadIdx.x];
  }
  for (uint32_t v = threadIdx.x; v < (tab->nbytes + 15) / 16; v += 256) reinterpret_cast<uint4*>(L.pat)[v] = reinterpret_cast<const uint4*>(tab->bytes)[v];
  const uint64_t a0 = g.src + p0 - g.pre;                                  // address of the tile's byte 0 (in front of src: the prefix)
  T.sh = (uint32_t)(a0 & 15u);
  const uint64_t s_lo = g.src + (p0 > g.pre ? p0 - g.pre : 0), s_hi = p0 + nbytes > g.pre ? g.src + min(g.len, p0 + nbytes - g.pre) : g.src;
  if (s_hi > s_lo) {
    const uint32_t nvec = (T.sh + nbytes + 15) / 16;
    for (uint32_t v = threadIdx.x; v < nvec; v += 256) {
      uint4 x = rg_ld16((a0 & ~15ull) + 16ull * v, s_lo, s_hi);
      if (fold) { x.x = sr_fold4(x.x); x.y = sr_fold4(x.y); x.z = sr_fold4(x.z); x.w = sr_fold4(x.w); }
      reinterpret_cast<uint4*>(L.text)[v] = x;
    }
  }
  __syncthreads();
  if (p0 < g.pre) {                                                          // the prefix: a few bytes of the carry buffer
    const uint32_t np = (uint32_t)min((uint64_t)nbytes, g.pre - p0);
    for (uint32_t j = threadIdx.x; j < np; j += 256) {
      uint8_t c = carry[p0 + j];
      if (fold && c >= 'A' && c <= 'Z') c += 32;
      reinterpret_cast<uint8_t*>(L.text)[T.sh + j] = c;
    }
  }
  __syncthreads();
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
  uint64_t run = 0;
  for (uint64_t b = 0; b < nt; b += 256) {
    const uint64_t i = b + threadIdx.x, v = i < nt ? cnt[i] : 0;
    uint64_t tot;
    const uint64_t ex = block_excl_sum<256, uint64_t>(v, sm, tot);
    if (i < nt) cnt[i] = run + ex;
    run += tot;
  }
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
  int cur = 0; uint32_t carry_len = 0; uint64_t carry_off = 0;     // carry_len bytes of decoded offset carry_off in buffer `cur`
  uint64_t h2d = 0, d2h = 0, tiles = 0;
  uint8_t* carry(int k) const { return (uint8_t*)mem.p + sizeof(SrPatTab) + SR_MAXL * (size_t)k; }

  int device_state() {                                             // (at the first batch: the device is current then)
    if (mem.p) return 0;
    mem = DevBuf(sizeof(SrPatTab) + 2 * SR_MAXL);
    if (!mem.p) return CJS_E_OUT_OF_MEMORY;
    if (hipMemcpy(mem.p, &tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) return CJS_E_HIP;
    h2d += sizeof tab;
    return 0;
  }

  // The matches of `segs` (npos set, in order), appended to the list.  Returns with the stream drained.
  int scan_segments(hipStream_t s, std::vector<SrSeg>& all) {
    std::vector<SrSeg> segs;
    uint64_t nt = 0;
    for (SrSeg g : all) if (g.npos) { g.tile0 = nt; nt += (g.npos + SR_TILE - 1) / SR_TILE; segs.push_back(g); }
    int rc = 0;
    if (nt) {
      if (nt > 0x7FFFFFFFull) return CJS_E_UNSUPPORTED;
      DevBuf d_segs(sizeof(SrSeg) * segs.size()), d_cnt(8 * (size_t)(nt + 1));
      if (!d_segs.p || !d_cnt.p) return CJS_E_OUT_OF_MEMORY;
      const SrPatTab* d_tab = (const SrPatTab*)mem.p;
      const uint32_t nseg = (uint32_t)segs.size();
      uint64_t total = 0;
      // from here on no way out without a synchronize: the copies may still be reading `segs` / writing `total`
      if (hipMemcpyAsync(d_segs.p, segs.data(), sizeof(SrSeg) * segs.size(), hipMemcpyHostToDevice, s) != hipSuccess) rc = CJS_E_HIP;
      else {
        hipLaunchKernelGGL(sr_count, dim3((unsigned)nt), dim3(256), 0, s, (const SrSeg*)d_segs.p, nseg, d_tab, (const uint8_t*)carry(cur), fold, win_lo, win_hi, (uint64_t*)d_cnt.p);
        hipLaunchKernelGGL(sr_scan, dim3(1), dim3(256), 0, s, (uint64_t*)d_cnt.p, nt);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&total, (uint64_t*)d_cnt.p + nt, 8, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
      }
      if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = CJS_E_HIP;
      if (rc) return rc;
      h2d += sizeof(SrSeg) * segs.size(); d2h += 8; tiles += nt;
      const uint64_t keep = n_matches < cap ? std::min<uint64_t>(total, cap - n_matches) : 0;
      if (keep) {                                                    // (a count query never gets here: one kernel pass less)
        DevBuf d_found(16 * (size_t)keep);
        if (!d_found.p) return CJS_E_OUT_OF_MEMORY;
        hipLaunchKernelGGL(sr_emit, dim3((unsigned)nt), dim3(256), 0, s, (const SrSeg*)d_segs.p, nseg, d_tab, (const uint8_t*)carry(cur), fold, win_lo, win_hi,
                           (const uint64_t*)d_cnt.p, (uint4*)d_found.p, keep);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(found + n_matches, d_found.p, 16 * (size_t)keep, hipMemcpyDeviceToHost, s) != hipSuccess) rc = CJS_E_HIP;
        if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = CJS_E_HIP;
        if (rc) return rc;
        d2h += 16 * keep;
      }
      n_matches += total;
      return 0;
    }
    return hipStreamSynchronize(s) != hipSuccess ? (int)CJS_E_HIP : 0;
  }

  SrSeg carry_segment() const { return SrSeg{0, 0, carry_off, carry_len, 0, carry_len, 0}; }      // the carry alone: nothing follows it

  // A decoded batch: its segments, the carry in front of the first if that goes on where the carry ends, else the carry on its
  // own; the last segment's tail becomes the new carry and is tested with the next batch (or by finish()).
  int batch(const RangeBatch& B, const std::vector<uint8_t>& verdict) {
    CJS_TRY(device_state());
    std::vector<SrSeg> segs;
    bool open = false, first = true;
    uint64_t end = 0;
    for (size_t k = B.g0; k < B.g1; k++) {
      const uint32_t b = B.blk[k];
      if (verdict[b] != RG_GOOD) { open = false; continue; }
      const uint64_t o = ix->off[b], len = ix->e[b].size;
      if (open && o == end) { segs.back().len += len; end += len; continue; }
      SrSeg g{(uint64_t)(uintptr_t)(B.d_exp + B.J.out_off[k]), len, o, 0, 0, 0, 0};
      if (first && carry_len) {
        if (carry_off + carry_len == o) { g.pre = carry_len; g.off = carry_off; }
        else segs.push_back(carry_segment());
      }
      first = false;
      segs.push_back(g); open = true; end = o + len;
    }
    if (first) return 0;                                             // no good block: the carry waits on
    for (SrSeg& g : segs) g.npos = g.pre + g.len;
    SrSeg& last = segs.back();
    const uint64_t n = last.pre + last.len, hold = std::min<uint64_t>(tab.maxlen - 1, n);
    last.npos = n - hold;
    int rc = 0;
    if (hold) {                                                      // bytes [n - hold, n) of the prefix and the segment
      uint8_t* to = carry(cur ^ 1);
      const uint64_t from_pre = n - hold < last.pre ? last.pre - (n - hold) : 0;
      if (from_pre && hipMemcpyAsync(to, carry(cur) + (last.pre - from_pre), (size_t)from_pre, hipMemcpyDeviceToDevice, B.s) != hipSuccess) rc = CJS_E_HIP;
      if (!rc && hold > from_pre &&
          hipMemcpyAsync(to + from_pre, (const uint8_t*)(uintptr_t)last.src + (last.len - (hold - from_pre)), (size_t)(hold - from_pre), hipMemcpyDeviceToDevice, B.s) != hipSuccess) rc = CJS_E_HIP;
    }
    const uint64_t new_off = last.off + n - hold;
    const int rc2 = scan_segments(B.s, segs);
    if (rc || rc2) { (void)hipStreamSynchronize(B.s); return rc ? rc : rc2; }
    cur ^= hold ? 1 : 0; carry_len = (uint32_t)hold; carry_off = new_off;
    return 0;
  }

  int finish() {                                                     // what still waits in the carry
    if (!carry_len) return 0;
    Stream s;
    if (hipStreamCreate(s.put()) != hipSuccess) return CJS_E_HIP;
    std::vector<SrSeg> segs(1, carry_segment());
    const int rc = scan_segments(s, segs);
    carry_len = 0;
    return rc;
  }
};

int search_check_args(const void* in, size_t n, const cjs_bz_index* idx, const uint8_t* pat, const uint32_t* pat_off, uint32_t npat, uint32_t flags,
                      const cjs_bz_match* found, size_t cap, const cjs_bz_search_info* info, SrPatTab& tab) {
  if (!idx || !info || !pat || !pat_off || (!in && n) || (!found && cap)) return CJS_E_INVALID_ARG;
  if (idx->stream_bytes != n) { set_detail("the index is of a stream of %llu bytes", (unsigned long long)idx->stream_bytes); return CJS_E_INVALID_ARG; }
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
  const uint64_t total = idx->off.back(), win_hi = off + len < off ? total : std::min<uint64_t>(off + len, total);
  std::vector<uint32_t> touched;                                   // the blocks of non-zero size that overlap [off, win_hi)
  if (off < win_hi)
    for (size_t b = range_block_of(idx, off); b < idx->e.size() && idx->off[b] < win_hi; b++) if (idx->e[b].size) touched.push_back((uint32_t)b);
  if (touched.empty()) return 0;
  CJS_TRY(select_device(opts));
  int ndev = 0, dev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CJS_E_NO_DEVICE;
  RestoreDevice restore{dev};
  if (d_in && !on_device(d_in, dev)) return CJS_E_INVALID_ARG;      // (no host pointer reaches a kernel)
  C.ix = idx; C.fold = flags & CJS_SEARCH_NOCASE; C.win_lo = off; C.win_hi = win_hi; C.found = found; C.cap = cap;
  std::vector<uint8_t> verdict(idx->e.size(), RG_GOOD); std::vector<uint32_t> crc_got(idx->e.size(), 0);
  RangeStats st;
  CJS_TRY(range_engine(in, d_in, idx, touched, verdict, crc_got, dev, st, [&](const RangeBatch& B) { return C.batch(B, verdict); }));
  CJS_TRY(C.finish());
  info->n_matches = C.n_matches; info->blocks_decoded = touched.size();
  for (uint32_t b : touched) if (verdict[b] != RG_GOOD) { if (!info->n_bad_blocks++) info->first_bad_block = b; }
  if (info->n_bad_blocks) range_bad_detail(idx, (size_t)info->first_bad_block, verdict, crc_got);
  if (env_debug())
    fprintf(stderr, "[cjs search] %s: %u patterns (longest %u), window [%llu, %llu), %zu of %zu blocks touched, %llu bad, %u passes (%u row batches, %u inverse-BWT batches), "
            "upload %llu B, %llu tiles, H2D %llu D2H %llu, %llu matches\n", d_in ? "device" : "host", npat, C.tab.maxlen, (unsigned long long)off, (unsigned long long)win_hi,
            touched.size(), idx->e.size(), (unsigned long long)info->n_bad_blocks, st.passes, st.a_batches, st.b_batches, (unsigned long long)st.up,
            (unsigned long long)C.tiles, (unsigned long long)(st.h2d + C.h2d), (unsigned long long)(st.d2h + C.d2h), (unsigned long long)C.n_matches);
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
