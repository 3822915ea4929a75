// range_engine.h -- the pass engine of the indexed entry points (range.hip defines it): the blocks an index names go through phases
// A, B and C in bounded passes, each judged against its entry, and every decoded inverse-BWT batch is handed to a consumer while it
// stands expanded in device scratch.  Seven consumers:
//   range.hip     the slice gather of the range reads
//   search.hip    the pattern scan: count, scan and emit over the tiles of a batch's segments, a carry between batches
//   regex.hip     the same scan with an automaton walk per start position as the match function (the tile's text: scan_text.h)
//   lines.hip     the newline count per block, select and rank for the line table's questions
//                 (its newline test, ln_nl4, stands here: the compressor's block rows, enc_index.hip, count with it too)
//   compare.hip   count, scan and emit over the tiles of the batch's runs intersected with the other side's
//   linekeys.hip  a key per line: count and hash per tile, a chain per block, a record per newline at its rank (line_key.h, line_join.h;
//                 tally_stream.hip runs it with the records kept on the device)
//   cut.hip       fields or byte columns of the lines: a summary per tile, one chain over the batch from the state the batch in
//                 front left, count, scan, and a byte-granular compaction through LDS (cut_plan.h)
// What they share stands here: the device helpers of a tile (its segment, its span of bounded aligned vectors, the 16-byte funnel,
// the byte tests over 16 bytes, the scan of the tile counts) and, on the host, the verdicts of a call, the check of a stream
// against its index and the count-then-emit round of the search and the compare.  Their host arithmetic (windows, runs,
// segments, the search's carry, the routing of a line question, a window of lines) is scan_plan.h, which includes no HIP.
#pragma once
#include "dec_engine.h"
#include "bz_index.h"
#include "prims.hpp"
#include "scan_plan.h"
#include <functional>
#include <vector>

namespace cjs {

enum { RG_GOOD = 0, RG_MISMATCH = 1, RG_BAD_CRC = 2 };      // a touched block against its index entry

// ---------------------------------------------------------------- device helpers
// The aligned 16 bytes at address p of a source that is bytes [lo, hi): a vector load when they all belong to it; at the two ends
// of a source the bytes that do, one by one, zeros for the others (nothing outside the source is read).
__device__ __forceinline__ uint4 rg_ld16(uint64_t p, uint64_t lo, uint64_t hi) {
  if (p >= lo && p + 16 <= hi) return *reinterpret_cast<const uint4*>(p);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 16; i++) if (p + i >= lo && p + i < hi) w[i >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(p + i) << (8 * (i & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// The 16 bytes at d = 16 q + 4 K + m of a source that is bytes [lo, hi): dword j is dwords K + j and K + j + 1 of the two aligned
// vectors that cover them, funnelled by m bytes.  Both loads are bounded to the source; bytes outside read as zeros.
template <int K>
__device__ __forceinline__ uint4 rg_funnel16(uint64_t d, uint32_t m, uint64_t lo, uint64_t hi) {
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

// the last of segs[0 .. nseg) with tile0 <= t (segs[0].tile0 is 0)
template <typename Seg, typename T>
__device__ __forceinline__ Seg rg_seg_of(const Seg* __restrict__ segs, uint32_t nseg, T t) {
  uint32_t lo = 0, hi = nseg;
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (segs[mid].tile0 <= t) lo = mid; else hi = mid; }
  return segs[lo];
}

// The bytes [a0, a0 + n) of a tile as aligned 16-byte vectors: vector v is the 16 bytes at base + 16 v, those outside the tile
// read as zeros (rg_ld16: nothing outside the tile is read).  Byte 0 of the tile is byte a0 & 15 of vector 0: the tile's phase.
struct RgSpan { uint64_t a0, base; uint32_t n, nvec; };
__device__ __forceinline__ RgSpan rg_span(uint64_t a0, uint32_t n) { return RgSpan{a0, a0 & ~15ull, n, ((uint32_t)(a0 & 15u) + n + 15u) / 16u}; }
__device__ __forceinline__ uint4 rg_vec(const RgSpan& S, uint32_t v) { return rg_ld16(S.base + 16ull * v, S.a0, S.a0 + S.n); }

// test4(w) sets bit 7 of every byte of w that passes, nothing else.  The bytes of the 16 that pass: their number, and bit i = byte i.
template <uint32_t (*test4)(uint32_t)>
__device__ __forceinline__ uint32_t rg_count16(uint4 x) { return __popc(test4(x.x)) + __popc(test4(x.y)) + __popc(test4(x.z)) + __popc(test4(x.w)); }
template <uint32_t (*test4)(uint32_t)>
__device__ __forceinline__ uint32_t rg_mask16(uint4 x) {
  auto nib = [](uint32_t z) { return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u); };
  return nib(test4(x.x)) | (nib(test4(x.y)) << 4) | (nib(test4(x.z)) << 8) | (nib(test4(x.w)) << 12);
}

// bit 7 of every byte of w that is 0x0A, nothing else: the exact zero-byte test (the borrow form flags a 0x0B behind a 0x0A too)
__device__ __forceinline__ uint32_t ln_nl4(uint32_t w) {
  const uint32_t v = w ^ 0x0A0A0A0Au, t = (v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  return ~(t | v | 0x7F7F7F7Fu);
}
// the newlines of 16 bytes: their number, and bit i = byte i is one
__device__ __forceinline__ uint32_t ln_count16(uint4 x) { return rg_count16<ln_nl4>(x); }
__device__ __forceinline__ uint32_t ln_mask16(uint4 x) { return rg_mask16<ln_nl4>(x); }

// One workgroup of 256: cnt[0 .. nt) -> their exclusive prefix sums; returns the total.  also(i) runs for every i < nt in front of
// its element's step.  sm: four words of LDS.
template <typename F>
__device__ __forceinline__ uint64_t rg_scan_counts(uint64_t* __restrict__ cnt, uint64_t nt, uint64_t* sm, F also) {
  uint64_t run = 0;
  for (uint64_t b = 0; b < nt; b += 256) {
    const uint64_t i = b + threadIdx.x, v = i < nt ? cnt[i] : 0;
    if (i < nt) also(i);
    uint64_t tot;
    const uint64_t ex = block_excl_sum<256, uint64_t>(v, sm, tot);
    if (i < nt) cnt[i] = run + ex;
    run += tot;
  }
  return run;
}

// ---------------------------------------------------------------- the engine
struct RangeStats { uint64_t h2d = 0, d2h = 0, up = 0; uint32_t passes = 0, a_batches = 0, b_batches = 0; size_t slices = 0; };

// The verdicts of a call, per block of the index: RG_*, and the computed CRC of an RG_BAD_CRC block.  The engine writes those of
// the touched blocks.
struct BadBlocks { uint64_t n = 0, first = ~0ull; };
struct RangeVerdicts {
  std::vector<uint8_t> verdict; std::vector<uint32_t> crc_got;
  explicit RangeVerdicts(const cjs_bz_index* ix) : verdict(ix->e.size(), RG_GOOD), crc_got(ix->e.size(), 0) {}
  bool good(size_t b) const { return verdict[b] == RG_GOOD; }
  BadBlocks bad_among(const std::vector<uint32_t>& touched) const {
    BadBlocks r;
    for (uint32_t b : touched) if (!good(b)) { if (!r.n++) r.first = b; }
    return r;
  }
  void set_bad_detail(const cjs_bz_index* ix, size_t bad) const;      // the detail text of bad block `bad`: one of read_ranges' two
};

// One decoded batch of a pass: chain blocks [g0, g1), chain block k being index block blk[k], out_len bytes at byte J.out_off[k]
// of d_exp (a block of the wrong size or with a bad CRC takes its room there all the same), its verdict already in V.
// q: scratch for the batch's duration; s: the pass's stream.
struct RangeBatch {
  const DecJob& J; DecShare& S; const std::vector<uint32_t>& blk; const RangeVerdicts& V;
  size_t g0, g1; uint8_t* d_exp; ShareScratch& q; hipStream_t s;
  uint64_t addr(size_t k) const { return (uint64_t)(uintptr_t)(d_exp + J.out_off[k]); }      // where chain block k stands
  // the batch's good blocks under [win_lo, win_hi) as runs (scan_plan.h); off: the index's decoded offsets
  std::vector<ScanRun> good_runs(const std::vector<uint64_t>& off, uint64_t win_lo, uint64_t win_hi) const {
    std::vector<uint64_t> at(g1 - g0);
    for (size_t k = g0; k < g1; k++) at[k - g0] = addr(k);
    return cjs::good_runs(blk.data() + g0, at.data(), g1 - g0, V.verdict, off, win_lo, win_hi);
  }
};
// returns with the stream drained
using RangeConsumer = std::function<int(const RangeBatch&)>;
// rc, or CJS_E_HIP if rc is 0 and stream s does not drain: a consumer's way out once something may be in flight
inline int drained(hipStream_t s, int rc) { return hipStreamSynchronize(s) != hipSuccess && !rc ? (int)CJS_E_HIP : rc; }

// in: the stream on the host, or nullptr with d_src: the stream on device `dev`.  touched: the blocks to decode, ascending.
int range_engine(const uint8_t* in, const uint8_t* d_src, const cjs_bz_index* ix, const std::vector<uint32_t>& touched, RangeVerdicts& V, int dev,
                 RangeStats& st, const RangeConsumer& consume);
// The range reads on the engine, the result in device memory: range k ([off[k], off[k] + len[k]) clipped to total_bytes) at d_out +
// the sum of the clipped lengths in front of it, from the stream on the host (`in`) or on device `dev` (d_src).  The region of a
// range that touches a bad block holds unspecified bytes; the verdicts say which blocks were bad.
int range_read_to_device(const uint8_t* in, const uint8_t* d_src, const cjs_bz_index* ix, const uint64_t* off, const uint64_t* len, size_t count,
                         uint8_t* d_out, RangeVerdicts& V, int dev, RangeStats& st);
// the block that holds decoded offset o < total_bytes (of non-zero size)
inline size_t range_block_of(const cjs_bz_index* ix, uint64_t o) { return block_of(ix->off, o); }
// n bytes at `in` (host or device) can be the stream of idx: CJS_E_INVALID_ARG, for another size with a detail text
int check_index_stream(const void* in, size_t n, const cjs_bz_index* idx);

// One count-then-emit round of a consumer on stream s, over nt tiles (none: nothing but the synchronize).  count_scan(cnt)
// enqueues the consumer's uploads and its count and scan kernels, which leave in cnt (nt + trail words of device memory) the
// exclusive prefix sums of the tile counts, their total and trail - 1 words more; it returns 0 or an error code.  The trailing
// words come back in res.  If room > 0 and the total > 0, emit(cnt, out, keep) enqueues the kernel that writes the first keep =
// min(total, room) 16-byte records, which are copied to host_out.  st: tiles and the bytes of these copies (count_scan adds its
// uploads).  Returns with the stream drained on every path.
struct ScanStats { uint64_t h2d = 0, d2h = 0, tiles = 0; };
int count_then_emit(hipStream_t s, uint64_t nt, uint32_t trail, const std::function<int(uint64_t* cnt)>& count_scan,
                    const std::function<void(const uint64_t* cnt, uint4* out, uint64_t keep)>& emit, void* host_out, uint64_t room, ScanStats& st, uint64_t* res);

}  // namespace cjs
