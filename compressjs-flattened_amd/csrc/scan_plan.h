// scan_plan.h -- host arithmetic of the consumers of the pass engine (range_engine.h): the window of a call and the blocks under
// it, the good blocks of a decoded batch as runs, two sides' runs as tiled segments (compare.hip), a batch's segments with the carry
// between batches (search.hip), where a line question is answered (lines.hip) and a window of lines with its touched blocks (cut.hip,
// linekeys.hip, tally_stream.hip, sort_stream.hip; the cut's own arithmetic is cut_plan.h).  Plain integers and vectors: offsets, sizes,
// verdict bytes, device addresses as uint64_t.  No HIP in here (tests/host/scan_plan_check.cc compiles it with the host compiler).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace cjs {

// ---------------------------------------------------------------- windows and blocks
// Block k of an index holds decoded bytes [off[k], off[k + 1]); off has one value more than there are blocks, the last the total.

// the end of [off, off + len) clipped to `total` (a sum that overflows reaches to the end)
inline uint64_t window_end(uint64_t off, uint64_t len, uint64_t total) { return off + len < off ? total : std::min(off + len, total); }
// the block that holds decoded offset o < off.back() (of non-zero size)
inline size_t block_of(const std::vector<uint64_t>& off, uint64_t o) { return (size_t)(std::upper_bound(off.begin(), off.end(), o) - off.begin()) - 1; }
// the blocks of non-zero size that overlap [lo, hi), hi <= off.back(), ascending
inline std::vector<uint32_t> blocks_under(const std::vector<uint64_t>& off, uint64_t lo, uint64_t hi) {
  std::vector<uint32_t> t;
  if (lo < hi)
    for (size_t b = block_of(off, lo); b + 1 < off.size() && off[b] < hi; b++) if (off[b + 1] > off[b]) t.push_back((uint32_t)b);
  return t;
}

// ---------------------------------------------------------------- runs and segments
struct ScanRun { uint64_t lo, hi, addr; };      // decoded bytes [lo, hi) at device address addr

// The good ones (verdict 0) of blocks blk[0 .. n), block blk[i]'s first byte at addr[i], clipped to [win_lo, win_hi): runs in the
// order of the blocks, two merged where the second goes on both where the first ends and at the address behind it.  A bad block
// and one with nothing inside the window give nothing.
inline std::vector<ScanRun> good_runs(const uint32_t* blk, const uint64_t* addr, size_t n, const std::vector<uint8_t>& verdict,
                                      const std::vector<uint64_t>& off, uint64_t win_lo, uint64_t win_hi) {
  std::vector<ScanRun> runs;
  for (size_t i = 0; i < n; i++) {
    const uint32_t b = blk[i];
    if (verdict[b] != 0) continue;
    const uint64_t lo = std::max(off[b], win_lo), hi = std::min(off[b + 1], win_hi);
    if (lo >= hi) continue;
    const uint64_t a = addr[i] + (lo - off[b]);
    if (!runs.empty() && runs.back().hi == lo && runs.back().addr + (runs.back().hi - runs.back().lo) == a) runs.back().hi = hi;
    else runs.push_back(ScanRun{lo, hi, a});
  }
  return runs;
}

// len bytes at device address a against those at b; decoded offset; first tile (the compare's kernels read these)
struct RunPair { uint64_t a, b, len, off, tile0; };
struct RunPairs { std::vector<RunPair> segs; uint64_t tiles = 0, bytes = 0; };
// mine intersected with theirs (each sorted, without overlap): a segment per overlap, in order, its tiles numbered densely
inline RunPairs intersect_runs(const std::vector<ScanRun>& mine, const std::vector<ScanRun>& theirs, uint64_t tile) {
  RunPairs P;
  for (const ScanRun& r : mine) {
    auto it = std::upper_bound(theirs.begin(), theirs.end(), r.lo, [](uint64_t o, const ScanRun& q) { return o < q.hi; });      // the first run that ends behind r.lo
    for (; it != theirs.end() && it->lo < r.hi; ++it) {
      const uint64_t lo = std::max(r.lo, it->lo), hi = std::min(r.hi, it->hi);
      if (lo >= hi) continue;
      P.segs.push_back(RunPair{r.addr + (lo - r.lo), it->addr + (lo - it->lo), hi - lo, lo, P.tiles});
      P.tiles += (hi - lo + tile - 1) / tile; P.bytes += hi - lo;
    }
  }
  return P;
}

// ---------------------------------------------------------------- the search's segments
// A segment of the search: len bytes at device address src behind `pre` bytes of the carry buffer, the first of all these bytes at
// decoded offset off; start positions [0, npos) of the pre + len bytes are tested (the search's kernels read these).
struct SearchSeg { uint64_t src, len, off, npos, tile0; uint32_t pre, pad; };
// The carry: the last len (< the longest pattern) bytes in front of decoded offset off + len, not yet tested as start positions.
struct SearchCarry { uint32_t len = 0; uint64_t off = 0; };
inline SearchSeg carry_segment(const SearchCarry& c) { return SearchSeg{0, 0, c.off, c.len, 0, c.len, 0}; }      // the carry alone: nothing follows it

// A batch's runs as segments: the carry in front of the first if that goes on where the carry ends, else the carry on its own.
// The last `hold` bytes of the last segment (longest - 1, or all it has) are not tested now; they become the next carry: from_pre
// bytes from the end of the old one, then hold - from_pre from the end of the segment.  No run: no segment, the carry waits on.
struct SearchPlan { std::vector<SearchSeg> segs; uint64_t hold = 0, from_pre = 0; SearchCarry next; };
inline SearchPlan search_plan(const std::vector<ScanRun>& runs, const SearchCarry& carry, uint32_t longest) {
  SearchPlan P;
  P.next = carry;
  if (runs.empty()) return P;
  for (const ScanRun& r : runs) {
    SearchSeg g{r.addr, r.hi - r.lo, r.lo, 0, 0, 0, 0};
    if (P.segs.empty() && carry.len) {
      if (carry.off + carry.len == r.lo) { g.pre = carry.len; g.off = carry.off; }
      else P.segs.push_back(carry_segment(carry));
    }
    P.segs.push_back(g);
  }
  for (SearchSeg& g : P.segs) g.npos = g.pre + g.len;
  SearchSeg& last = P.segs.back();
  const uint64_t n = last.pre + last.len;
  P.hold = std::min<uint64_t>(longest - 1, n);
  last.npos = n - P.hold;
  P.from_pre = n - P.hold < last.pre ? last.pre - (n - P.hold) : 0;
  P.next = SearchCarry{(uint32_t)P.hold, last.off + n - P.hold};
  return P;
}
// the segments that test something, their tiles numbered densely; returns the number of tiles
inline uint64_t tile_segments(std::vector<SearchSeg>& segs, uint64_t tile) {
  uint64_t nt = 0;
  size_t kept = 0;
  for (SearchSeg g : segs) if (g.npos) { g.tile0 = nt; nt += (g.npos + tile - 1) / tile; segs[kept++] = g; }
  segs.resize(kept);
  return nt;
}

// ---------------------------------------------------------------- line questions
// Where a question of the line table is answered.  block == ~0: by the table alone, with `value`.  Else in block `block`, from its
// bytes: the arg-th newline of the block (locate, 1-based) or the newlines among its first arg bytes (number).
struct LineRoute { uint32_t block = ~0u, arg = 0; uint64_t value = 0; };
// cum: the newlines in front of block k (one value more than blocks: the last is their number N).  Line q starts behind newline q:
// line 0 at offset 0, a line past N at the end.
inline LineRoute route_locate(const std::vector<uint64_t>& cum, uint64_t total, uint64_t q) {
  LineRoute r;
  if (q == 0 || q > cum.back()) { r.value = q ? total : 0; return r; }
  const size_t b = (size_t)(std::lower_bound(cum.begin(), cum.end(), q) - cum.begin()) - 1;      // cum[b] < line <= cum[b+1]
  r.block = (uint32_t)b; r.arg = (uint32_t)(q - cum[b]);
  return r;
}
// the newlines in front of decoded offset q: all of them at or past the end, the table's own at a block's first byte
inline LineRoute route_number(const std::vector<uint64_t>& cum, const std::vector<uint64_t>& off, uint64_t q) {
  LineRoute r;
  if (q >= off.back()) { r.value = cum.back(); return r; }
  const size_t b = block_of(off, q);
  if (q == off[b]) { r.value = cum[b]; return r; }
  r.block = (uint32_t)b; r.arg = (uint32_t)(q - off[b]);
  return r;
}
// A window of lines [first, first + count) over N newlines (lines 0 .. N, the last the tail): its end (the add saturates) ...
inline uint64_t line_window_end(uint64_t first, uint64_t count, uint64_t N) { return first + count < first ? N + 1 : std::min(first + count, N + 1); }
// ... and the touched blocks of [first, end), end <= N + 1: the blocks of non-zero size from the block of newline number `first`
// through the block of newline number `end`, route_locate's answer for a line's start.  off: the blocks' sizes, as their offsets.
inline std::vector<uint32_t> line_window_blocks(const std::vector<uint64_t>& cum, uint64_t total_bytes, const std::vector<uint64_t>& off, uint64_t first, uint64_t end) {
  std::vector<uint32_t> touched;
  if (first >= end || cum.size() < 2) return touched;      // (an empty window; an empty index)
  const size_t b0 = first ? route_locate(cum, total_bytes, first).block : 0, b1 = end <= cum.back() ? route_locate(cum, total_bytes, end).block : cum.size() - 2;
  for (size_t b = b0; b <= b1; b++) if (off[b + 1] > off[b]) touched.push_back((uint32_t)b);
  return touched;
}

}  // namespace cjs
