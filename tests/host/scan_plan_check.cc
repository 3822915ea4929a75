// scan_plan_check.cc — the host arithmetic of csrc/scan_plan.h (windows and the blocks under them, the good blocks of a batch as
// runs, two sides' runs as tiled segments, the search's segments and carry, the routing of a line question, a window of lines and its
// touched blocks) checked by property on random cases against brute-force models, not by restating its formulas.  Stand-alone:
// built with the host compiler under the address / undefined-behaviour sanitizers and run by tests/test_scan_plan_host.py.  Exit 0 =
// all checks passed; a failing check prints itself and the program exits 1.
#include "scan_plan.h"
#include "cjs_hip.h"
#include <stdio.h>
#include <vector>

using namespace cjs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
typedef unsigned long long ull;

// An index of 1 .. 40 blocks, sizes 0 .. max_size (about one in four is 0), the first block at decoded offset 0.
static std::vector<uint64_t> random_offsets(uint64_t max_size) {
  std::vector<uint64_t> off(1, 0);
  for (size_t n = 1 + rnd() % 40; n; n--) off.push_back(off.back() + (rnd() % 4 == 0 ? 0 : 1 + rnd() % max_size));
  return off;
}
// byte o of the text -> its block, by walking the blocks
static size_t block_by_walk(const std::vector<uint64_t>& off, uint64_t o) {
  for (size_t b = 0; b + 1 < off.size(); b++) if (off[b] <= o && o < off[b + 1]) return b;
  return ~(size_t)0;
}

static void window_cases() {
  const uint64_t M = ~0ull;
  CHECK(window_end(5, M, 100) == 100 && window_end(M, M, 100) == 100 && window_end(M - 1, 2, 100) == 100, "an overflowing off + len reaches to the end");
  CHECK(window_end(5, 10, 100) == 15 && window_end(5, 95, 100) == 100 && window_end(5, 96, 100) == 100 && window_end(5, 0, 100) == 5, "clamp");
  CHECK(window_end(200, 5, 100) == 100 && window_end(7, M - 7, M) == M && window_end(7, M - 6, M) == M, "past the end");
  for (int it = 0; it < 4000; it++) {
    const std::vector<uint64_t> off = random_offsets(1 + rnd() % 9);
    const uint64_t total = off.back();
    const uint64_t lo = rnd() % (total + 3), len = rnd() % 5 == 0 ? M - rnd() % 3 : rnd() % (total + 3), hi = window_end(lo, len, total);
    CHECK(hi <= total && (lo + len < lo || hi == std::min(lo + len, total)), "window_end(%llu, %llu, %llu) = %llu", (ull)lo, (ull)len, (ull)total, (ull)hi);
    const std::vector<uint32_t> got = blocks_under(off, lo, hi);
    std::vector<uint32_t> want;                                     // the blocks that hold a byte of [lo, hi)
    for (uint64_t o = lo; o < hi; o++) { const size_t b = block_by_walk(off, o); if (want.empty() || want.back() != b) want.push_back((uint32_t)b); }
    CHECK(got == want, "blocks_under [%llu, %llu) of %zu blocks: %zu blocks, expected %zu", (ull)lo, (ull)hi, off.size() - 1, got.size(), want.size());
    if (total) { const uint64_t o = rnd() % total; CHECK(block_of(off, o) == block_by_walk(off, o), "block_of(%llu)", (ull)o); }
  }
}

// A batch of blocks of an index: some of its blocks in ascending order, each at an address; the blocks stand packed in the order of
// the batch (a bad block takes its room), with a gap in front of a block now and then if `gaps`.
struct Batch { std::vector<uint32_t> blk; std::vector<uint64_t> addr; };
static Batch random_batch(const std::vector<uint64_t>& off, size_t b0, size_t b1, bool zero_sized, bool gaps, uint64_t base) {
  Batch B;
  uint64_t at = base;
  for (size_t b = b0; b < b1; b++) {
    if (off[b + 1] == off[b] && !zero_sized) continue;
    if (gaps && rnd() % 5 == 0) at += 1 + rnd() % 40;
    B.blk.push_back((uint32_t)b); B.addr.push_back(at);
    at += off[b + 1] - off[b];
  }
  return B;
}

static void good_run_cases() {
  for (int it = 0; it < 4000; it++) {
    const std::vector<uint64_t> off = random_offsets(1 + rnd() % 9);
    const size_t nb = off.size() - 1;
    std::vector<uint8_t> verdict(nb);
    for (auto& v : verdict) v = rnd() % 4 == 0 ? (uint8_t)(1 + rnd() % 2) : 0;
    const Batch B = random_batch(off, 0, nb, true, it % 2 == 1, 0x1000 + rnd() % 16);
    const uint64_t total = off.back(), lo = it % 3 == 0 ? 0 : rnd() % (total + 2), hi = it % 3 == 0 ? ~0ull : window_end(lo, rnd() % (total + 2), total);
    const std::vector<ScanRun> runs = good_runs(B.blk.data(), B.addr.data(), B.blk.size(), verdict, off, lo, hi);
    // byte by byte: the window's bytes of the good blocks, each with its address, in order
    std::vector<std::pair<uint64_t, uint64_t>> want, got;
    for (size_t i = 0; i < B.blk.size(); i++) {
      const uint32_t b = B.blk[i];
      if (verdict[b]) continue;
      for (uint64_t o = off[b]; o < off[b + 1]; o++) if (o >= lo && o < hi) want.push_back({o, B.addr[i] + (o - off[b])});
    }
    for (const ScanRun& r : runs) {
      CHECK(r.lo < r.hi, "an empty run [%llu, %llu)", (ull)r.lo, (ull)r.hi);
      for (uint64_t o = r.lo; o < r.hi; o++) got.push_back({o, r.addr + (o - r.lo)});
    }
    CHECK(got == want, "good_runs: %zu bytes in %zu runs, expected %zu bytes", got.size(), runs.size(), want.size());
    for (size_t k = 1; k < runs.size(); k++) {                      // ascending, no overlap, and merged wherever they could be
      CHECK(runs[k - 1].hi <= runs[k].lo, "runs %zu and %zu overlap or descend", k - 1, k);
      CHECK(!(runs[k - 1].hi == runs[k].lo && runs[k - 1].addr + (runs[k - 1].hi - runs[k - 1].lo) == runs[k].addr), "runs %zu and %zu are adjacent in offset and address but not merged", k - 1, k);
    }
  }
}

static std::vector<ScanRun> random_runs(uint64_t span, uint64_t base) {
  std::vector<ScanRun> r;
  for (uint64_t o = rnd() % 8; o < span;) {
    const uint64_t len = 1 + rnd() % (rnd() % 4 == 0 ? 60000 : 300);
    r.push_back(ScanRun{o, o + len, base + o * 3 + rnd() % 16});
    o += len + (rnd() % 3 == 0 ? 0 : rnd() % 200);
  }
  return r;
}

static void intersect_cases() {
  for (int it = 0; it < 3000; it++) {
    const uint64_t span = 1 + rnd() % (it % 10 == 0 ? 100000 : 5000), tile = it % 4 == 0 ? 64 : 16384;
    const std::vector<ScanRun> mine = random_runs(span, 0x100000), theirs = it % 50 == 0 ? std::vector<ScanRun>() : random_runs(span, 0x9000000);
    const RunPairs P = intersect_runs(mine, theirs, tile);
    // the bytes both sides have, from a map of every byte of `theirs`
    std::vector<uint64_t> their_addr(theirs.empty() ? 0 : (size_t)theirs.back().hi, 0);      // (0: theirs has no such byte)
    for (const ScanRun& r : theirs) for (uint64_t o = r.lo; o < r.hi; o++) their_addr[o] = r.addr + (o - r.lo);
    std::vector<uint64_t> want_o, want_a, want_b, got_o, got_a, got_b;
    for (const ScanRun& r : mine) for (uint64_t o = r.lo; o < r.hi; o++) if (o < their_addr.size() && their_addr[o]) { want_o.push_back(o); want_a.push_back(r.addr + (o - r.lo)); want_b.push_back(their_addr[o]); }
    uint64_t tiles = 0, bytes = 0;
    for (const RunPair& g : P.segs) {
      CHECK(g.len > 0 && g.tile0 == tiles, "segment at %llu: len %llu, tile0 %llu, expected %llu", (ull)g.off, (ull)g.len, (ull)g.tile0, (ull)tiles);
      tiles += (g.len + tile - 1) / tile; bytes += g.len;
      for (uint64_t i = 0; i < g.len; i++) { got_o.push_back(g.off + i); got_a.push_back(g.a + i); got_b.push_back(g.b + i); }
    }
    CHECK(P.tiles == tiles && P.bytes == bytes && bytes == want_o.size(), "tiles %llu (%llu), bytes %llu (%llu, %zu)", (ull)P.tiles, (ull)tiles, (ull)P.bytes, (ull)bytes, want_o.size());
    CHECK(got_o == want_o && got_a == want_a && got_b == want_b, "intersect_runs: the segments are not mine and theirs byte by byte, in order");
  }
}

// The search over a whole call: random blocks, verdicts, cuts into batches and a longest pattern.  Every segment is looked at
// position by position against the good runs of the whole text.
static void search_cases(uint32_t max_pattern) {
  for (int it = 0; it < 3000; it++) {
    const uint32_t longest = it % 7 == 0 ? max_pattern : it % 7 == 1 ? 1 : 1 + (uint32_t)(rnd() % (it % 2 ? 12 : max_pattern));
    const std::vector<uint64_t> off = random_offsets(it % 3 == 0 ? 3 : 1 + rnd() % (it % 8 == 1 ? 2 * longest + 4 : longest / 2 + 4));
    const size_t nb = off.size() - 1;
    std::vector<uint8_t> verdict(nb);
    for (auto& v : verdict) v = rnd() % 5 == 0 ? (uint8_t)(1 + rnd() % 2) : 0;
    // run_end[o]: where the good run that holds byte o ends (0: o is in no good block); zero-size blocks belong to no batch
    std::vector<uint64_t> run_end(off.back(), 0);
    for (size_t b = nb; b-- > 0;) {
      if (verdict[b] || off[b + 1] == off[b]) continue;
      const uint64_t end = off[b + 1] < off.back() && run_end[off[b + 1]] ? run_end[off[b + 1]] : off[b + 1];
      for (uint64_t o = off[b]; o < off[b + 1]; o++) run_end[o] = end;
    }
    std::vector<uint32_t> tested(off.back(), 0);
    SearchCarry carry;
    auto look = [&](std::vector<SearchSeg>& segs, const SearchCarry& had) {
      const uint64_t tile = 64;
      std::vector<SearchSeg> all = segs;
      const uint64_t nt = tile_segments(segs, tile);
      uint64_t tiles = 0; size_t k = 0;
      for (const SearchSeg& g : all) {
        if (!g.npos) continue;
        CHECK(k < segs.size() && segs[k].tile0 == tiles && segs[k].off == g.off && segs[k].npos == g.npos && segs[k].pre == g.pre && segs[k].len == g.len, "tile_segments: segment %zu", k);
        tiles += (g.npos + tile - 1) / tile; k++;
      }
      CHECK(k == segs.size() && nt == tiles, "tile_segments: %zu segments of %zu, %llu tiles of %llu", segs.size(), k, (ull)nt, (ull)tiles);
      for (const SearchSeg& g : all) {
        CHECK(g.npos <= g.pre + g.len, "npos %llu of %u + %llu bytes", (ull)g.npos, g.pre, (ull)g.len);
        if (g.pre) CHECK(g.pre == had.len && g.off == had.off, "a prefix of %u bytes at %llu, the carry has %u at %llu", g.pre, (ull)g.off, had.len, (ull)had.off);
        for (uint64_t i = 0; i < g.npos && g.off + i < tested.size(); i++) {
          const uint64_t p = g.off + i, behind = g.pre + g.len - i - 1;
          tested[p]++;
          CHECK(run_end[p] != 0, "position %llu is tested but in no good block", (ull)p);
          CHECK(behind >= std::min<uint64_t>(longest - 1, run_end[p] - p - 1), "position %llu has %llu bytes behind it, its run %llu, longest %u", (ull)p, (ull)behind, (ull)(run_end[p] - p - 1), longest);
          CHECK(p + behind < run_end[p], "the segment of position %llu reaches past its good run", (ull)p);
        }
      }
    };
    for (size_t b0 = 0; b0 < nb;) {
      const size_t b1 = std::min(nb, b0 + 1 + (size_t)(rnd() % 6));
      const Batch B = random_batch(off, b0, b1, false, false, 0x4000 + 4096 * b0 + rnd() % 16);
      const std::vector<ScanRun> runs = good_runs(B.blk.data(), B.addr.data(), B.blk.size(), verdict, off, 0, ~0ull);
      SearchPlan P = search_plan(runs, carry, longest);
      if (runs.empty()) CHECK(P.segs.empty() && P.next.len == carry.len && P.next.off == carry.off && !P.hold, "a batch without a good block changes the carry");
      else {
        const SearchSeg& last = P.segs.back();
        CHECK(P.next.len == P.hold && P.hold <= longest - 1 && P.next.off + P.next.len == runs.back().hi, "carry of %u bytes at %llu, hold %llu, the last run ends at %llu, longest %u", P.next.len, (ull)P.next.off,
              (ull)P.hold, (ull)runs.back().hi, longest);
        CHECK(last.npos + P.hold == last.pre + last.len, "the last segment tests %llu and holds %llu of %u + %llu", (ull)last.npos, (ull)P.hold, last.pre, (ull)last.len);
        // the held bytes are the last of the prefix and the segment: all the segment can give, the rest from the end of the prefix
        CHECK(P.from_pre <= last.pre && P.hold - P.from_pre <= last.len && (P.from_pre == 0 || P.hold - P.from_pre == last.len), "hold %llu = %llu of the prefix (%u) + the rest of the segment (%llu)",
              (ull)P.hold, (ull)P.from_pre, last.pre, (ull)last.len);
        size_t k = 0;                                                // the segments are the runs, the carry in or in front of the first
        if (!P.segs[0].len) { CHECK(carry.len && P.segs[0].pre == carry.len && P.segs[0].npos == carry.len && carry.off + carry.len != runs[0].lo, "a carry on its own"); k = 1; }
        else if (carry.len) CHECK(P.segs[0].pre == carry.len && carry.off + carry.len == runs[0].lo, "a carry of %u bytes is dropped", carry.len);
        CHECK(P.segs.size() == k + runs.size(), "%zu segments for %zu runs", P.segs.size(), runs.size());
        for (size_t r = 0; r < runs.size() && k + r < P.segs.size(); r++) {
          const SearchSeg& g = P.segs[k + r];
          CHECK(g.src == runs[r].addr && g.len == runs[r].hi - runs[r].lo && g.off + g.pre == runs[r].lo && (r == 0 || g.pre == 0), "segment %zu is not run %zu", k + r, r);
        }
      }
      look(P.segs, carry);
      carry = P.next;
      b0 = b1;
    }
    if (carry.len) { std::vector<SearchSeg> segs(1, carry_segment(carry)); look(segs, carry); }      // the final flush
    for (uint64_t o = 0; o < tested.size(); o++) CHECK(tested[o] == (run_end[o] ? 1u : 0u), "position %llu tested %u times (good: %d), longest %u", (ull)o, tested[o], run_end[o] != 0, longest);
  }
}

static void line_cases() {
  for (int it = 0; it < 4000; it++) {
    const std::vector<uint64_t> off = random_offsets(1 + rnd() % 9);
    const size_t nb = off.size() - 1;
    std::vector<uint64_t> cum(1, 0); std::vector<uint32_t> nl_block;      // nl_block[j]: the block of newline j + 1
    for (size_t b = 0; b < nb; b++) {
      const uint64_t nl = rnd() % 3 == 0 ? 0 : rnd() % (off[b + 1] - off[b] + 1);
      for (uint64_t j = 0; j < nl; j++) nl_block.push_back((uint32_t)b);
      cum.push_back(cum.back() + nl);
    }
    const uint64_t N = cum.back(), total = off.back();
    for (uint64_t q = 0; q <= N + 2; q++) {
      const LineRoute r = route_locate(cum, total, q == N + 2 ? ~0ull : q);
      if (q == 0) CHECK(r.block == ~0u && r.value == 0, "line 0 starts at 0");
      else if (q > N) CHECK(r.block == ~0u && r.value == total, "a line past the last starts at the end");
      else {
        uint32_t first = 0;                                          // the first newline of that block
        while (nl_block[first] != nl_block[q - 1]) first++;
        CHECK(r.block == nl_block[q - 1] && r.arg == q - first, "line %llu: block %u arg %u, expected block %u arg %llu", (ull)q, r.block, r.arg, nl_block[q - 1], (ull)(q - first));
      }
    }
    for (uint64_t q = 0; q <= total + 2; q++) {
      const LineRoute r = route_number(cum, off, q == total + 2 ? ~0ull : q);
      const size_t b = q < total ? block_by_walk(off, q) : 0;
      uint64_t before = 0;                                           // the newlines of the blocks in front of b
      for (uint32_t x : nl_block) before += x < b;
      if (q >= total) CHECK(r.block == ~0u && r.value == N, "an offset at or past the end has every newline in front of it");
      else if (q == off[b]) CHECK(r.block == ~0u && r.value == before, "offset %llu starts block %zu: %llu, expected %llu", (ull)q, b, (ull)r.value, (ull)before);
      else CHECK(r.block == b && r.arg == q - off[b], "offset %llu: block %u arg %u, expected block %zu arg %llu", (ull)q, r.block, r.arg, b, (ull)(q - off[b]));
    }
  }
}

// The window of lines and its touched blocks, against a walk over the text itself: line q starts behind newline q, the blocks that
// hold a byte of the window's lines are touched, and so is every block from the start of a line to its end.
static void line_window_cases() {
  const uint64_t M = ~0ull;
  CHECK(line_window_end(0, M, 7) == 8 && line_window_end(3, M - 2, 7) == 8 && line_window_end(M, M, 7) == 8 && line_window_end(5, 0, 7) == 5, "the add saturates");
  CHECK(line_window_end(2, 3, 7) == 5 && line_window_end(2, 6, 7) == 8 && line_window_end(2, 7, 7) == 8 && line_window_end(9, 1, 7) == 8 && line_window_end(0, 0, 0) == 0, "clamp to N + 1");
  const std::vector<uint64_t> none_cum(1, 0), none_off(1, 0);
  CHECK(line_window_blocks(none_cum, 0, none_off, 0, 1).empty(), "an empty index has no block to touch");
  for (int it = 0; it < 4000; it++) {
    // blocks with empty ones at either end now and then; a text over them with a newline about every fifth byte
    std::vector<uint64_t> off = random_offsets(1 + rnd() % 9);
    if (it % 3 == 0) off.insert(off.begin(), 1 + rnd() % 2, 0);
    if (it % 3 == 1) off.insert(off.end(), 1 + rnd() % 2, off.back());
    const size_t nb = off.size() - 1;
    const uint64_t total = off.back();
    std::vector<uint8_t> is_nl(total);
    for (auto& x : is_nl) x = rnd() % 5 == 0;
    if (it % 7 == 0) std::fill(is_nl.begin(), is_nl.end(), 0);
    std::vector<uint64_t> cum(1, 0), start(1, 0);                     // start[q]: the offset line q starts at
    for (size_t b = 0; b < nb; b++) {
      uint64_t c = 0;
      for (uint64_t o = off[b]; o < off[b + 1]; o++) if (is_nl[o]) { c++; start.push_back(o + 1); }
      cum.push_back(cum.back() + c);
    }
    const uint64_t N = cum.back();
    start.push_back(total);                                           // (where the line behind the tail would start)
    for (int w = 0; w < 6; w++) {
      const uint64_t first = w == 0 ? 0 : w == 1 ? N + 1 + rnd() % 3 : rnd() % (N + 2);
      const uint64_t count = w == 2 ? 0 : w == 3 ? M : rnd() % (N + 3), end = line_window_end(first, count, N);
      CHECK(end <= N + 1 && (first + count < first || end == std::min(first + count, N + 1)), "line_window_end(%llu, %llu, %llu) = %llu", (ull)first, (ull)count, (ull)N, (ull)end);
      const std::vector<uint32_t> got = line_window_blocks(cum, total, off, first, end);
      // per line of the window: the block its start lies in (an empty line at the very end starts in the last block with bytes),
      // and every block up to the one its last byte lies in
      std::vector<uint8_t> want(nb, 0);
      for (uint64_t q = first; q < end; q++) {
        const uint64_t lo = start[q], hi = start[q + 1];              // the line's bytes [lo, hi)
        if (!total) break;
        const size_t b0 = block_by_walk(off, std::min(lo, total - 1)), b1 = block_by_walk(off, hi > lo ? hi - 1 : std::min(lo, total - 1));
        for (size_t b = b0; b <= b1; b++) if (off[b + 1] > off[b]) want[b] = 1;
      }
      std::vector<uint32_t> want_list;
      for (size_t b = 0; b < nb; b++) if (want[b]) want_list.push_back((uint32_t)b);
      // the routing reads a line's start from the block of the newline in front of it: that block may come in front of the brute
      // force's first, never behind it, and nothing else differs
      std::vector<uint32_t> extra;
      for (uint32_t b : got) if (!want[b]) extra.push_back(b);
      for (uint32_t b : want_list) CHECK(std::find(got.begin(), got.end(), b) != got.end(), "lines [%llu, %llu): block %u holds a byte of the window and is not touched", (ull)first, (ull)end, b);
      CHECK(std::is_sorted(got.begin(), got.end()) && std::adjacent_find(got.begin(), got.end()) == got.end(), "touched blocks ascend without repeats");
      for (uint32_t b : got) CHECK(off[b + 1] > off[b], "block %u of size zero is touched", b);
      CHECK(extra.size() <= 1, "lines [%llu, %llu): %zu blocks touched beyond those that hold the window", (ull)first, (ull)end, extra.size());
      if (extra.size() == 1) {
        // the one block more: the newline in front of the window's first line is the last byte of a block and the line starts in the next
        CHECK(first > 0 && first <= N && extra[0] == block_by_walk(off, start[first] - 1) && (want_list.empty() || extra[0] < want_list[0]),
              "lines [%llu, %llu): block %u is touched and neither holds a byte of the window nor the newline in front of it", (ull)first, (ull)end, extra[0]);
      }
      if (first >= end) CHECK(got.empty(), "an empty window touches %zu blocks", got.size());
    }
  }
}

int main() {
  window_cases();
  good_run_cases();
  intersect_cases();
  search_cases(CJS_SEARCH_MAX_PATTERN_BYTES);
  line_cases();
  line_window_cases();
  if (g_fail) { printf("scan_plan_check: %d checks failed\n", g_fail); return 1; }
  printf("scan_plan_check ok\n");
  return 0;
}
