// line_key_check.cc -- csrc/line_key.h and csrc/line_diff.h on the CPU (tests/test_line_key_host_check.py builds this with the host
// compiler under the address and undefined-behaviour sanitizers and runs it; no HIP, nothing loaded into Python).
//   the mulmod, the power and the join against naive 128-bit arithmetic; the join's associativity on random splits of random
//   strings; the keys of a text against a byte-by-byte restatement
//   the diff against the quadratic DP on random pairs, na and nb in {0, 1} included, and on pairs whose recursion ends on every
//   branch (an insertion, a deletion, an empty range, a split at a snake of length zero)
#include "line_diff.h"
#include "line_key.h"
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

using namespace cjs;
typedef unsigned __int128 u128;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { if (fails++ < 20) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static uint64_t naive_mul(uint64_t a, uint64_t b) { return (uint64_t)((u128)a * b % LK_P); }
static uint64_t naive_pow(uint64_t b, uint64_t n) { uint64_t r = 1; for (uint64_t i = 0; i < n; i++) r = naive_mul(r, b); return r; }
static LkFrag naive_frag(const std::string& s, const LkBases& B) {
  u128 h1 = 0, h2 = 0;
  for (unsigned char c : s) { h1 = (h1 * B.b1 + c + 1) % LK_P; h2 = (h2 * B.b2 + c + 1) % LK_P; }
  return LkFrag{(uint64_t)h1, (uint64_t)h2, s.size()};
}
static bool same(const LkFrag& a, const LkFrag& b) { return a.h1 == b.h1 && a.h2 == b.h2 && a.len == b.len; }
static LkFrag frag_of(const std::string& s, const LkBases& B) { LkFrag f{0, 0, 0}; for (unsigned char c : s) lk_push(f, B, c); return f; }

static void check_arithmetic() {
  const uint64_t edge[] = {0, 1, 2, 255, 256, LK_P - 1, LK_P - 2, 1ull << 60, (1ull << 60) + 1, 1ull << 32, (1ull << 32) - 1, 0x1555555555555555ull};
  for (uint64_t a : edge) for (uint64_t b : edge) CHECK(lk_mul(a, b) == naive_mul(a, b));
  for (int i = 0; i < 200000; i++) { const uint64_t a = rnd() % LK_P, b = rnd() % LK_P; CHECK(lk_mul(a, b) == naive_mul(a, b)); CHECK(lk_add(a, b) == (a + b) % LK_P); }
  for (int i = 0; i < 300; i++) { const uint64_t b = rnd() % LK_P, n = rnd() % 700; CHECK(lk_pow(b, n) == naive_pow(b, n)); }
  CHECK(lk_pow(12345, 0) == 1 && lk_pow(0, 0) == 1 && lk_pow(0, 5) == 0);
  // the bases: splitmix64's first two outputs for state 0 are published values
  uint64_t st = 0;
  CHECK(lk_splitmix(st) == 0xE220A8397B1DCDAFull && lk_splitmix(st) == 0x6E789E6AA1B965F4ull);
  const LkBases B0 = lk_bases(0);
  CHECK(B0.b1 == 256 + 0xE220A8397B1DCDAFull % (LK_P - 256) && B0.b2 == 256 + 0x6E789E6AA1B965F4ull % (LK_P - 256));
}

static void check_join() {
  for (int round = 0; round < 400; round++) {
    const LkBases B = lk_bases(rnd());
    CHECK(B.b1 >= 256 && B.b1 < LK_P && B.b2 >= 256 && B.b2 < LK_P);
    std::string s((size_t)(rnd() % 200), '\0');
    for (char& c : s) c = (char)(rnd() % 4 == 0 ? (rnd() % 2 ? 0 : 255) : rnd());
    const LkFrag whole = naive_frag(s, B);
    CHECK(same(frag_of(s, B), whole));
    // any two cuts: (x | y) | z == x | (y | z) == the whole
    size_t c1 = (size_t)(rnd() % (s.size() + 1)), c2 = (size_t)(rnd() % (s.size() + 1));
    if (c1 > c2) std::swap(c1, c2);
    const LkFrag x = frag_of(s.substr(0, c1), B), y = frag_of(s.substr(c1, c2 - c1), B), z = frag_of(s.substr(c2), B);
    CHECK(same(lk_join(lk_join(x, y, B), z, B), whole));
    CHECK(same(lk_join(x, lk_join(y, z, B), B), whole));
    const LkFrag none{0, 0, 0};
    CHECK(same(lk_join(none, whole, B), whole) && same(lk_join(whole, none, B), whole));
    CHECK(whole.h1 < LK_P && whole.h2 < LK_P);
  }
  const LkBases B = lk_bases(7);
  CHECK(frag_of("", B).h1 == 0 && frag_of(std::string(1, '\0'), B).h1 == 1 && frag_of(std::string(2, '\0'), B).h1 == (B.b1 + 1) % LK_P);
  // the keys of a text: one per newline and the tail; cap is kept
  const std::string text = std::string("ab\n\n") + std::string(3, '\0') + "\nxyz";
  cjs_bz_linekey k[8];
  for (auto& e : k) e = lk_bad_key();
  CHECK(lk_text_keys((const uint8_t*)text.data(), text.size(), 7, k, 3) == 4);
  CHECK(lk_is_bad(k[3]) && !lk_is_bad(k[2]));
  CHECK(lk_text_keys((const uint8_t*)text.data(), text.size(), 7, k, 8) == 4);
  const char* want[4] = {"ab\n", "\n", "\0\0\0\n", "xyz"};
  const size_t wlen[4] = {3, 1, 4, 3};
  for (int i = 0; i < 4; i++) {
    const LkFrag f = naive_frag(std::string(want[i], wlen[i]), B);
    CHECK(k[i].hash == f.h1 && k[i].len == wlen[i] && k[i].check == (uint32_t)f.h2);
  }
  CHECK(lk_same(k[0], k[0]) && !lk_same(k[0], k[1]) && !lk_same(lk_bad_key(), lk_bad_key()));
  CHECK(lk_text_keys(nullptr, 0, 7, k, 8) == 1 && k[0].hash == 0 && k[0].len == 0 && k[0].check == 0);
}

typedef std::vector<int> Seq;
static std::vector<cjs_bz_linekey> keys_of(const Seq& s) {
  std::vector<cjs_bz_linekey> k(s.size());
  for (size_t i = 0; i < s.size(); i++) k[i] = s[i] < 0 ? lk_bad_key() : cjs_bz_linekey{(uint64_t)s[i] * 977 + 1, (uint32_t)s[i], (uint32_t)s[i] * 31};
  return k;
}
static uint64_t dp_edits(const Seq& a, const Seq& b) {
  std::vector<std::vector<uint32_t>> l(a.size() + 1, std::vector<uint32_t>(b.size() + 1, 0));
  for (size_t i = 1; i <= a.size(); i++)
    for (size_t j = 1; j <= b.size(); j++)
      l[i][j] = (a[i - 1] == b[j - 1] && a[i - 1] >= 0) ? l[i - 1][j - 1] + 1 : std::max(l[i - 1][j], l[i][j - 1]);
  return a.size() + b.size() - 2 * (uint64_t)l[a.size()][b.size()];
}
// the script is well formed and turns a into b; returns its edits
static uint64_t check_script(const Seq& a, const Seq& b, const std::vector<cjs_bz_hunk>& h, const cjs_bz_ldiff_info& info) {
  Seq out;
  uint64_t at = 0, edits = 0;
  int64_t shift = 0;
  for (size_t i = 0; i < h.size(); i++) {
    CHECK(h[i].a_count || h[i].b_count);
    CHECK((int64_t)h[i].b_first == (int64_t)h[i].a_first + shift);
    CHECK(i == 0 || h[i].a_first > h[i - 1].a_first + h[i - 1].a_count);
    CHECK(h[i].a_first >= at && h[i].a_first + h[i].a_count <= a.size() && h[i].b_first + h[i].b_count <= b.size());
    if (h[i].a_first < at || h[i].a_first + h[i].a_count > a.size() || h[i].b_first + h[i].b_count > b.size()) return ~0ull;
    out.insert(out.end(), a.begin() + (long)at, a.begin() + (long)h[i].a_first);
    out.insert(out.end(), b.begin() + (long)h[i].b_first, b.begin() + (long)(h[i].b_first + h[i].b_count));
    at = h[i].a_first + h[i].a_count;
    shift += (int64_t)h[i].b_count - (int64_t)h[i].a_count;
    edits += h[i].a_count + h[i].b_count;
  }
  out.insert(out.end(), a.begin() + (long)at, a.end());
  CHECK(out == b);
  CHECK(info.n_hunks == h.size() && info.edits == edits && info.common == (a.size() + b.size() - edits) / 2 && info.reserved == 0);
  return edits;
}
static void check_pair(const Seq& a, const Seq& b, uint64_t max_edits) {
  const std::vector<cjs_bz_linekey> ka = keys_of(a), kb = keys_of(b);
  cjs_bz_ldiff_info info, info2;
  CHECK(lk_diff(ka.data(), ka.size(), kb.data(), kb.size(), max_edits, nullptr, 0, &info) == 0);
  std::vector<cjs_bz_hunk> h((size_t)info.n_hunks + 1, cjs_bz_hunk{~0ull, ~0ull, ~0ull, ~0ull});
  CHECK(lk_diff(ka.data(), ka.size(), kb.data(), kb.size(), max_edits, h.data(), (size_t)info.n_hunks, &info2) == 0);
  CHECK(h.back().a_first == ~0ull && info2.n_hunks == info.n_hunks && info2.edits == info.edits && info2.minimal == info.minimal);
  h.pop_back();
  const uint64_t edits = check_script(a, b, h, info), least = dp_edits(a, b);
  const uint64_t cap = max_edits ? max_edits : LK_DIFF_DEFAULT_MAX_EDITS;
  CHECK((info.minimal == 1) == (least <= cap));
  if (info.minimal) CHECK(edits == least);
  else CHECK(h.size() == 1 && edits >= least);
}

static void check_diff() {
  // both sizes in {0, 1}, equal and not
  for (int na = 0; na < 2; na++) for (int nb = 0; nb < 2; nb++) for (int eq = 0; eq < 2; eq++) check_pair(Seq((size_t)na, 1), Seq((size_t)nb, eq ? 1 : 2), 0);
  // the recursion's ends: insertion only, deletion only, both halves empty, a snake of length zero (nothing common at all), the
  // bad record on both sides
  check_pair({1, 2, 3}, {1, 9, 2, 3}, 0); check_pair({1, 9, 2, 3}, {1, 2, 3}, 0); check_pair({1, 2}, {3, 4}, 0); check_pair({1, 2, 3}, {4, 5}, 0);
  check_pair({1, 2, 3, 4}, {2, 1, 4, 3}, 0); check_pair({1, -1, 2}, {1, -1, 2}, 0); check_pair({5, 1, 2, 3, 6}, {7, 1, 2, 3, 8}, 0);
  check_pair({1, 2, 3, 4, 5, 6}, {6, 5, 4, 3, 2, 1}, 0);
  for (int round = 0; round < 3000; round++) {
    const size_t na = (size_t)(rnd() % 60), nb = (size_t)(rnd() % 60);
    const int alphabet = 1 + (int)(rnd() % 6);
    Seq a(na), b(nb);
    for (int& x : a) x = (int)(rnd() % (uint64_t)alphabet);
    for (int& x : b) x = (int)(rnd() % (uint64_t)alphabet);
    if (round % 4 == 0) {                                    // b is a with a few edits
      b = a;
      for (int e = (int)(rnd() % 6); e > 0; e--) {
        const size_t p = (size_t)(rnd() % (b.size() + 1));
        if (rnd() % 2 && !b.empty()) b.erase(b.begin() + (long)std::min(p, b.size() - 1));
        else b.insert(b.begin() + (long)p, (int)(rnd() % (uint64_t)alphabet));
      }
    }
    check_pair(a, b, 0);
    check_pair(a, b, 1 + rnd() % 40);                        // a cap on either side of the minimum
  }
}

int main() {
  check_arithmetic();
  check_join();
  check_diff();
  if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
  printf("line_key_check ok\n");
  return 0;
}
