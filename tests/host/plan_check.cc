// plan_check.cc — the host arithmetic of csrc/dec_plan.h (row layout, row batches, a streaming step's row limit, inverse-BWT batches
// and their slot plan) checked by property, not by restating its formulas.  Stand-alone: built with the host compiler under the
// address / undefined-behaviour sanitizers and run by tests/test_plan_host.py.  Exit 0 = all checks passed; a failing check prints
// itself and the program exits 1.
#include "dec_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace cjs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

struct C { uint64_t bit; uint32_t kind, pad; };      // the fields of Cand

// 0 .. 200 candidates at ascending bits, kind 1 with probability p1 / 8, block rows numbered in pad as phase A does
static std::vector<C> random_cands(uint32_t p1) {
  std::vector<C> v(rnd() % 201);
  uint64_t bit = 32; uint32_t row = 0;
  for (auto& c : v) { bit += 1 + rnd() % 5000; c.bit = bit; c.kind = rnd() % 8 < p1; c.pad = c.kind == 0 ? row++ : 0u; }
  return v;
}

static void batch_cut_cases() {
  for (int it = 0; it < 4000; it++) {
    const std::vector<C> v = random_cands((uint32_t)(it % 9));
    const uint32_t n = (uint32_t)v.size(), nr = 1 + (uint32_t)(rnd() % 5);
    uint32_t c0 = 0, next_row = 0, guard = 0;
    while (c0 < n && guard++ <= n) {
      const RowBatch b = row_batch(v.data(), n, c0, nr);
      CHECK(b.c0 == c0 && b.c1 > c0 && b.c1 <= n, "cut [%u, %u) from %u of %u", b.c0, b.c1, c0, n);      // in order, no gap, never empty
      if (b.c1 <= c0) return;
      uint32_t rows = 0, first = ~0u;
      for (uint32_t c = c0; c < b.c1; c++) if (v[c].kind == 0) { if (first == ~0u) first = v[c].pad; rows++; }
      CHECK(rows == b.rows && rows <= nr, "rows %u counted %u nr %u", b.rows, rows, nr);
      if (rows) CHECK(b.r0 == first && first == next_row, "r0 %u first row %u expected %u", b.r0, first, next_row);
      next_row += rows;
      // full unless it is the last; the end-of-stream candidates behind its last block go with it
      if (b.c1 < n) CHECK(rows == nr && v[b.c1].kind == 0, "batch [%u, %u) ends early: rows %u of %u, next kind %u", c0, b.c1, rows, nr, v[b.c1].kind);
      c0 = b.c1;
    }
    CHECK(c0 == n, "batches end at %u of %u", c0, n);
  }
}

static void row_limit_cases() {
  for (int it = 0; it < 4000; it++) {
    const std::vector<C> v = random_cands((uint32_t)(it % 9));
    const uint64_t row_from = v.empty() ? 0 : (rnd() % 4 == 0 ? 0 : v[rnd() % v.size()].bit + rnd() % 3 - 1);
    const uint32_t limit = rnd() % 8 == 0 ? ~0u : (uint32_t)(rnd() % 12);
    std::vector<C> t = v;
    const uint64_t cut = row_limit_trim(t, row_from, limit);
    if (limit == ~0u) {
      CHECK(cut == ~0ull && t.size() == v.size(), "no limit: cut %llx, %zu of %zu left", (unsigned long long)cut, t.size(), v.size());
      for (size_t i = 0; i < t.size() && i < v.size(); i++) CHECK(t[i].bit == v[i].bit && t[i].kind == v[i].kind && t[i].pad == v[i].pad, "no limit: candidate %zu changed", i);
      continue;
    }
    // what survives is one contiguous run of v, from the first candidate at or behind row_from on
    size_t a = 0;
    while (a < v.size() && v[a].bit < row_from) a++;
    uint32_t blocks = 0;
    for (size_t i = 0; i < t.size(); i++) {
      CHECK(a + i < v.size() && t[i].bit == v[a + i].bit && t[i].kind == v[a + i].kind, "survivor %zu is not candidate %zu", i, a + i);
      CHECK(t[i].bit >= row_from, "survivor at bit %llu in front of %llu", (unsigned long long)t[i].bit, (unsigned long long)row_from);
      blocks += t[i].kind == 0;
    }
    CHECK(blocks <= limit, "%u blocks survive a limit of %u", blocks, limit);
    const size_t end = a + t.size();                 // the first dropped candidate behind the survivors, if any
    if (end < v.size()) {
      CHECK(v[end].kind == 0 && blocks == limit && cut == v[end].bit, "cut %llx at candidate %zu (kind %u, bit %llu), %u of %u blocks", (unsigned long long)cut, end,
            v[end].kind, (unsigned long long)v[end].bit, blocks, limit);
    } else CHECK(cut == ~0ull, "nothing dropped behind the survivors, cut %llx", (unsigned long long)cut);
  }
}

static const uint32_t COUNTS[] = {1, 2, 63, 64, 65, 99999, 100000, 900000};
static void ib_plan_cases() {
  const uint32_t rs_tile = 4096;
  for (int it = 0; it < 1500; it++) {
    const uint32_t nb = 1 + (uint32_t)(rnd() % 300);
    std::vector<uint32_t> cnt(nb);
    const uint32_t uniform = COUNTS[rnd() % 8];
    const int mode = it % 3;                          // uniform / uniform but for a short last block / mixed
    for (uint32_t k = 0; k < nb; k++) cnt[k] = mode == 2 ? COUNTS[rnd() % 8] : uniform;
    if (mode == 1) cnt[nb - 1] = 1 + (uint32_t)(rnd() % uniform);
    const IbPlan P = ib_plan(nb, rs_tile, [&](uint32_t k) { return cnt[k]; });
    uint64_t sum = 0; uint32_t maxc = 0;
    for (uint32_t k = 0; k < nb; k++) { CHECK(P.woff[k] == (uint32_t)sum, "woff[%u] %u, running sum %llu", k, P.woff[k], (unsigned long long)sum); sum += cnt[k]; if (cnt[k] > maxc) maxc = cnt[k]; }
    CHECK(P.M64 == sum && P.maxc == maxc && P.nb == nb, "M64 %llu sum %llu maxc %u %u", (unsigned long long)P.M64, (unsigned long long)sum, P.maxc, maxc);
    CHECK(P.fits() == (sum < 0xFFFFF000ull), "fits");
    if (!P.fits()) continue;
    CHECK(P.M < 0xFFFFF000u, "M %u", P.M);
    // the parent's two inequalities on the segment size (the largest count, up to a multiple of four)
    const uint64_t slots = (uint64_t)nb * ((maxc + 3u) & ~3u);
    CHECK(P.strided == (slots <= sum + sum / 4 && slots < 0xFFFFF000ull), "strided %d: %llu slots for %llu elements", (int)P.strided, (unsigned long long)slots, (unsigned long long)sum);
    // slot ranges [off, off + count), in block order, disjoint, inside M; a strided block starts on its segment and fits it
    uint64_t prev_end = 0;
    for (uint32_t k = 0; k < nb; k++) {
      CHECK(P.off[k] >= prev_end && (uint64_t)P.off[k] + cnt[k] <= P.M, "block %u: slots [%u, +%u) behind %llu inside %u", k, P.off[k], cnt[k], (unsigned long long)prev_end, P.M);
      prev_end = (uint64_t)P.off[k] + cnt[k];
      if (P.strided) CHECK(P.off[k] == k * P.seg_stride && cnt[k] <= P.seg_stride && P.seg_stride % 4 == 0, "block %u: segment at %u, stride %u", k, P.off[k], P.seg_stride);
    }
    if (!P.strided) CHECK(P.M == sum, "back to back: M %u for %llu elements", P.M, (unsigned long long)sum);
    // the radix tiles cover every slot (a segment's, segment by segment), a splitter row holds the largest block's splitters and the start entry
    CHECK((uint64_t)P.tps * rs_tile >= P.seg_stride, "tps %u", P.tps);
    CHECK(P.strided ? P.T >= (size_t)nb * P.tps : (uint64_t)P.T * rs_tile >= P.M, "T %zu", P.T);
    CHECK(P.spl_stride >= (maxc + SPL - 1) / SPL + 1, "spl_stride %u for %u", P.spl_stride, maxc);
  }
}

static void ib_batch_cases() {
  for (int it = 0; it < 2000; it++) {
    const size_t n = rnd() % 400;
    std::vector<uint32_t> cnt(n);
    for (auto& c : cnt) c = COUNTS[rnd() % 8];
    uint64_t max_el = 1 + rnd() % 3000000;
    if (n && it % 2) { max_el = 0; for (size_t k = rnd() % n, e = k + 1 + rnd() % 4; k < n && k < e; k++) max_el += cnt[k]; }      // a limit some run of blocks meets exactly
    const size_t max_blocks = 1 + rnd() % 100;
    size_t b0 = 0;
    while (b0 < n) {
      const size_t b1 = ib_batch_end(b0, n, max_el, max_blocks, [&](size_t k) { return cnt[k]; });
      CHECK(b1 > b0 && b1 <= n && b1 - b0 <= max_blocks, "batch [%zu, %zu) of %zu, <= %zu blocks", b0, b1, n, max_blocks);
      if (b1 <= b0) return;
      uint64_t el = 0;
      for (size_t k = b0; k < b1; k++) el += cnt[k];
      CHECK(el <= max_el || b1 == b0 + 1, "batch [%zu, %zu): %llu elements, limit %llu", b0, b1, (unsigned long long)el, (unsigned long long)max_el);
      if (b1 < n) CHECK(b1 - b0 == max_blocks || el + cnt[b1] > max_el, "batch [%zu, %zu) could take block %zu", b0, b1, b1);      // greedy
      b0 = b1;
    }
  }
}

static void row_layout_cases() {
  const size_t tab = 18000;                           // (about a RowTab)
  for (int it = 0; it < 20000; it++) {
    const uint32_t dsz = 100000u * (1 + (uint32_t)(rnd() % 9));
    const uint32_t nrows = rnd() % 4 == 0 ? (uint32_t)(rnd() % 3) : (uint32_t)(rnd() % 200000);
    const RowLayout L0 = row_layout(dsz, 1, ~0ull, 256, tab);
    const uint64_t budget = rnd() % 8 == 0 ? rnd() % (2 * L0.per_row) : rnd() % (70000 * L0.per_row);
    const RowLayout L = row_layout(dsz, nrows, budget, 256, tab);
    CHECK(L.nr >= 1 && L.nr <= 65535, "nr %u", L.nr);
    CHECK(L.per_row == L0.per_row, "per_row depends on the rows or the budget");
    if (budget >= L.per_row) CHECK((uint64_t)L.nr * L.per_row <= budget, "nr %u x %llu > budget %llu", L.nr, (unsigned long long)L.per_row, (unsigned long long)budget);
    CHECK(L.single == (nrows <= L.nr), "single %d: %u rows in batches of %u", (int)L.single, nrows, L.nr);
    CHECK(L.nr <= (nrows ? nrows : 1u), "nr %u for %u rows", L.nr, nrows);
    // a row holds a whole block of the level: its ops, a tile of slack, whole tiles; the symbols in whole groups
    CHECK(L.ops_stride >= dsz + 256 && L.ops_stride % 256 == 0 && L.tiles_per_row * 256 == L.ops_stride, "ops_stride %u tiles %u", L.ops_stride, L.tiles_per_row);
    CHECK(L.sym_stride >= dsz && (uint64_t)L.sym_groups * GROUP_SYMS >= L.sym_stride, "sym_stride %u groups %u", L.sym_stride, L.sym_groups);
    CHECK((uint64_t)L.group_tiles * 256 >= (L.sym_groups < MAX_SELECTORS ? L.sym_groups : MAX_SELECTORS), "group_tiles %u for %u groups", L.group_tiles, L.sym_groups);
  }
}

int main() {
  batch_cut_cases();
  row_limit_cases();
  ib_plan_cases();
  ib_batch_cases();
  row_layout_cases();
  if (g_fail) { printf("plan_check: %d checks failed\n", g_fail); return 1; }
  printf("plan_check ok\n");
  return 0;
}
