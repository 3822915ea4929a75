// sort_plan_check -- the rule of the line sort (csrc/sort_plan.h) on the host, without HIP: sl_word against a byte-wise
// restatement, sl_sort_host (the rounds) against std::stable_sort with memcmp on random texts, the flags, the caps, the tail rule
// and the argument errors.  A stand-alone program; the test builds it under the address and undefined-behaviour sanitizers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "sort_plan.h"

using namespace cjs;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 33) % n);
}

// the issue's definition, byte by byte
static uint64_t word_restated(const std::vector<uint8_t>& line, long d) {
  uint64_t w = 0;
  for (long i = 0; i < 7; i++) w = w << 8 | (d + i < (long)line.size() ? line[(size_t)(d + i)] : 0);
  long left = (long)line.size() - d;
  left = left < 0 ? 0 : left > 7 ? 7 : left;
  return w << 8 | (uint64_t)left;
}

static void check_words() {
  for (int fill = 0; fill < 3; fill++)
    for (long d = 0; d <= 21; d += 7)
      for (long rest = -2; rest <= 9; rest++) {
        const long len = d + rest;
        if (len < 0) continue;
        std::vector<uint8_t> line((size_t)len + 16, fill == 0 ? 0x00 : 0xFF);      // (16 bytes behind the line: never part of the word)
        if (fill == 2) for (size_t i = 0; i < line.size(); i++) line[i] = (uint8_t)(i * 37 + 1);
        std::vector<uint8_t> only(line.begin(), line.begin() + len);
        const uint64_t w = sl_word(line.data(), (uint64_t)len, (uint64_t)d);
        CHECK(w == word_restated(only, d));
        CHECK((w & 0xFF) == (uint64_t)(rest < 0 ? 0 : rest > 7 ? 7 : rest));
        CHECK(sl_word_ended(w) == (rest < 7));
      }
  // padding sorts below a real 0x00: "ab" < "ab\0" < "ab\0\0" < "ab\1"
  const uint8_t a[] = {'a', 'b', 0, 0, 1};
  const uint8_t b[] = {'a', 'b', 1};
  CHECK(sl_word(a, 2, 0) < sl_word(a, 3, 0) && sl_word(a, 3, 0) < sl_word(a, 4, 0) && sl_word(a, 4, 0) < sl_word(b, 3, 0));
  CHECK(sl_max_rounds(0) == 1 && sl_max_rounds(5) == 1 && sl_max_rounds(6) == 2 && sl_max_rounds(4097) == 586);
}

struct Want { std::vector<uint64_t> lines, counts; cjs_bz_sort_info info; };

// std::stable_sort with memcmp over the lines, then the flags
static Want restated(const std::vector<uint8_t>& text, uint32_t flags) {
  std::vector<std::string> ln;
  size_t s = 0;
  for (size_t i = 0; i < text.size(); i++) if (text[i] == '\n') { ln.emplace_back((const char*)text.data() + s, i - s); s = i + 1; }
  if (s < text.size()) ln.emplace_back((const char*)text.data() + s, text.size() - s);
  std::vector<uint32_t> order(ln.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
  auto cmp = [&](uint32_t x, uint32_t y) {
    const size_t m = std::min(ln[x].size(), ln[y].size());
    const int c = m ? memcmp(ln[x].data(), ln[y].data(), m) : 0;
    return c ? c : (ln[x].size() < ln[y].size() ? -1 : ln[x].size() > ln[y].size() ? 1 : 0);
  };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cmp(x, y) < 0; });
  std::vector<std::vector<uint32_t>> runs;
  for (uint32_t i : order) { if (!runs.empty() && cmp(runs.back()[0], i) == 0) runs.back().push_back(i); else runs.push_back({i}); }
  Want w;
  sl_info_clear(&w.info);
  w.info.n_lines = ln.size(); w.info.n_distinct = runs.size();
  uint64_t deepest = 0;
  for (size_t k = 0; k + 1 < order.size(); k++) {
    const std::string &x = ln[order[k]], &y = ln[order[k + 1]];
    uint64_t c = 0;
    while (c < x.size() && c < y.size() && x[c] == y[c]) c++;
    deepest = std::max(deepest, c / 7);
  }
  w.info.rounds = ln.empty() ? 0 : 1 + deepest;
  if (flags & CJS_SORT_REVERSE) std::reverse(runs.begin(), runs.end());
  for (const auto& r : runs)
    for (size_t k = 0; k < ((flags & CJS_SORT_UNIQUE) ? 1 : r.size()); k++) {
      w.lines.push_back(r[k]); w.counts.push_back((flags & CJS_SORT_UNIQUE) ? r.size() : 1);
      w.info.text_bytes += ln[r[k]].size() + 1;
    }
  w.info.n_out = w.lines.size();
  return w;
}

static bool same_info(const cjs_bz_sort_info& a, const cjs_bz_sort_info& b) { return memcmp(&a, &b, sizeof a) == 0; }

static void check_text(const std::vector<uint8_t>& text) {
  for (uint32_t flags = 0; flags < 4; flags++) {
    const Want w = restated(text, flags);
    const size_t caps[] = {text.size() + 1, 0, 1, w.lines.size() ? w.lines.size() - 1 : 0, w.lines.size() + 5};
    for (size_t cap : caps) {
      std::vector<uint64_t> lines(cap + 1, ~0ull), counts(cap + 1, ~0ull);
      cjs_bz_sort_info info;
      CHECK(sl_sort_host(text.data(), text.size(), flags, lines.data(), cap & 1 ? counts.data() : nullptr, cap, &info) == 0);
      CHECK(same_info(info, w.info));
      CHECK(info.rounds <= sl_max_rounds(text.size()));
      const size_t m = std::min(cap, w.lines.size());
      for (size_t i = 0; i < m; i++) CHECK(lines[i] == w.lines[i] && (!(cap & 1) || counts[i] == w.counts[i]));
      for (size_t i = m; i <= cap; i++) CHECK(lines[i] == ~0ull && counts[i] == ~0ull);
    }
  }
}

static void check_sorts() {
  const uint32_t alphabets[] = {2, 3, 256};
  const uint32_t around[] = {0, 6, 7, 8, 14};
  for (int t = 0; t < 400; t++) {
    const uint32_t alpha = alphabets[t % 3], nlines = rnd(60);
    std::vector<uint8_t> text;
    for (uint32_t k = 0; k < nlines; k++) {
      const uint32_t base = around[rnd(5)], len = base ? base - 1 + rnd(3) : rnd(2);
      for (uint32_t i = 0; i < len; i++) {
        uint8_t c = alpha == 256 ? (uint8_t)rnd(256) : (uint8_t)("a\0\xFF"[rnd(alpha)]);
        if (c == '\n') c = 0x0B;
        text.push_back(c);
      }
      text.push_back('\n');
    }
    if (t % 4 == 0 && !text.empty()) text.pop_back();      // the tail without its newline
    if (t % 7 == 0) { text.push_back('a'); text.push_back('b'); }
    check_text(text);
  }
  // the tail rule, only newlines, no newline, equal lines, a proper prefix
  const std::string texts[] = {"", "\n", "\n\n\n", "x", "x\n", "x\ny", "b\na\nb\na", std::string("ab\x01\nab\0\0\nab\0\nab\n", 16), "abcdefg\nabcdefgh\nabcdefg\n",
                               "abcdefgabcdefg\nabcdefgabcdefg"};
  for (const std::string& str : texts) check_text(std::vector<uint8_t>(str.begin(), str.end()));
}

static void check_args() {
  const uint8_t text[] = {'b', '\n', 'a', '\n'};
  uint64_t lines[4], counts[4];
  cjs_bz_sort_info info;
  CHECK(sl_sort_host(text, 4, 0, lines, counts, 4, nullptr) == CJS_E_INVALID_ARG);
  CHECK(sl_sort_host(nullptr, 4, 0, lines, counts, 4, &info) == CJS_E_INVALID_ARG);
  CHECK(sl_sort_host(text, 4, 0, nullptr, counts, 4, &info) == CJS_E_INVALID_ARG);
  CHECK(sl_sort_host(text, 4, 4, lines, counts, 4, &info) == CJS_E_INVALID_ARG);
  CHECK(sl_sort_host(text, (size_t)SL_MAX_BYTES + 1, 0, nullptr, nullptr, 0, &info) == CJS_E_UNSUPPORTED);
  CHECK(sl_sort_host(nullptr, 0, 3, nullptr, nullptr, 0, &info) == 0 && info.n_lines == 0 && info.n_out == 0 && info.rounds == 0 && info.first_bad_block == ~0ull);
  CHECK(sl_sort_host(text, 4, 0, lines, nullptr, 4, &info) == 0 && lines[0] == 1 && lines[1] == 0 && info.text_bytes == 4);
  CHECK(sl_args(text, 4, 0, lines, 4, true, false, &info) == CJS_E_INVALID_ARG && sl_args(text, 4, 0, lines, 4, true, true, &info) == 0);
  CHECK(sl_flags_ok(3) && !sl_flags_ok(8));
  CHECK(sl_work_bytes(1000, 100000) == sl_count_bytes(100000) + sl_lines_bytes(1000) && sl_lines_bytes(0) == sl_lines_bytes(1));
  CHECK(sl_lines_bytes(1 << 20) >= 90ull << 20 && sl_lines_bytes(1 << 20) < 91ull << 20);
  CHECK(sizeof(cjs_bz_sort_info) == 64);
}

int main() {
  check_words();
  check_sorts();
  check_args();
  printf("sort_plan_check ok\n");
  return 0;
}
