// cut_plan_check.cc -- the arithmetic of the column cut (csrc/cut_plan.h) against naive restatements, on the CPU: the list parser with
// every refusal, the normal form, membership against a naive set, the associativity of the summary monoid on random three-way
// splits, the pieces of a text cut with the carried state against cut_text of the whole, the saturating counter, and cut_text
// against a second implementation written here (split the lines, split the fields, join).  A stand-alone program: it is built with
// the host compiler under the address and undefined-behaviour sanitizers and run (tests/test_cut_plan_host_check.py).
#include "cut_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using namespace cjs;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); if (++fails > 20) exit(1); } } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static uint32_t below(uint32_t n) { return rnd() % n; }

typedef std::vector<cjs_cut_range> Ranges;

static bool naive_member(const Ranges& r, uint32_t k) {
  for (const cjs_cut_range& q : r) if (k >= q.lo && k <= q.hi) return true;
  return false;
}
static bool has_below(const Ranges& r, uint32_t k) {
  for (const cjs_cut_range& q : r) if (q.lo < k) return true;
  return false;
}

// the second implementation: the lines, their fields or bytes, joined
static std::string naive_cut(const std::string& text, uint32_t mode, uint8_t d, const Ranges& r) {
  std::vector<std::string> lines;
  size_t at = 0;
  for (;;) {
    const size_t nl = text.find('\n', at);
    if (nl == std::string::npos) break;
    lines.push_back(text.substr(at, nl - at));
    at = nl + 1;
  }
  if (at < text.size()) lines.push_back(text.substr(at));      // the tail, if it is not empty
  std::string out;
  for (const std::string& ln : lines) {
    if (mode == CJS_CUT_BYTES) {
      for (size_t i = 0; i < ln.size(); i++) if (naive_member(r, (uint32_t)i + 1)) out.push_back(ln[i]);
    } else {
      std::vector<std::string> f(1);
      for (char c : ln) { if ((uint8_t)c == d) f.emplace_back(); else f.back().push_back(c); }
      bool any = false;
      for (size_t k = 0; k < f.size(); k++) {
        if (!naive_member(r, (uint32_t)k + 1)) continue;
        if (any) out.push_back((char)d);
        out += f[k]; any = true;
      }
    }
    out.push_back('\n');
  }
  return out;
}

static void check_parser() {
  cjs_cut_range r[8];
  uint32_t n = 0;
  CHECK(ct_parse_list("1,3-5,7-", r, 8, &n) == 0 && n == 3 && r[0].lo == 1 && r[0].hi == 1 && r[1].lo == 3 && r[1].hi == 5 && r[2].lo == 7 && r[2].hi == CT_TO_END);
  CHECK(ct_parse_list("-4", r, 8, &n) == 0 && n == 1 && r[0].lo == 1 && r[0].hi == 4);
  CHECK(ct_parse_list("9,2,2-3", r, 8, &n) == 0 && n == 3 && r[0].lo == 9 && r[2].hi == 3);      // (kept as written: the normal form sorts)
  CHECK(ct_parse_list("4294967294", r, 8, &n) == 0 && r[0].lo == 0xFFFFFFFEu && r[0].hi == 0xFFFFFFFEu);
  CHECK(ct_parse_list("1,2,3,4,5,6,7,8", r, 8, &n) == 0 && n == 8);
  const char* refused[] = {"", ",", "1,", ",1", "1,,2", "0", "0-3", "-0", "5-3", "-", "1--2", "1-2-3", "a", "1a", "1 ,2", " 1", "1-a", "+1", "4294967295",
                           "99999999999999999999", "1-4294967295", "1,2,3,4,5,6,7,8,9"};
  for (const char* s : refused) { n = 77; CHECK(ct_parse_list(s, r, 8, &n) == CJS_E_INVALID_ARG && n == 77); }
  CHECK(ct_parse_list(nullptr, r, 8, &n) == CJS_E_INVALID_ARG && ct_parse_list("1", r, 8, nullptr) == CJS_E_INVALID_ARG && ct_parse_list("1", nullptr, 8, &n) == CJS_E_INVALID_ARG);
  CHECK(ct_parse_list("1", r, 0, &n) == CJS_E_INVALID_ARG);
}

static Ranges random_ranges(uint32_t top) {
  Ranges r(1 + below(rnd() % 4 ? 4 : CT_MAX_RANGES));
  for (cjs_cut_range& q : r) {
    q.lo = 1 + below(top);
    q.hi = below(8) == 0 ? CT_TO_END : q.lo + below(below(3) ? 3 : top);
  }
  return r;
}

static void check_normal_form_and_membership() {
  CtSel S;
  cjs_cut_range one{1, 1};
  CHECK(ct_normalise(2, 9, &one, 1, &S) == CJS_E_INVALID_ARG && ct_normalise(CJS_CUT_FIELDS, 256, &one, 1, &S) == CJS_E_INVALID_ARG);
  CHECK(ct_normalise(CJS_CUT_FIELDS, 0x0A, &one, 1, &S) == CJS_E_INVALID_ARG && ct_normalise(CJS_CUT_BYTES, 0x0A, &one, 1, &S) == 0);
  CHECK(ct_normalise(CJS_CUT_FIELDS, 9, &one, 0, &S) == CJS_E_INVALID_ARG && ct_normalise(CJS_CUT_FIELDS, 9, nullptr, 1, &S) == CJS_E_INVALID_ARG);
  cjs_cut_range many[CT_MAX_RANGES + 1];
  for (cjs_cut_range& q : many) q = one;
  CHECK(ct_normalise(CJS_CUT_FIELDS, 9, many, CT_MAX_RANGES + 1, &S) == CJS_E_INVALID_ARG && ct_normalise(CJS_CUT_FIELDS, 9, many, CT_MAX_RANGES, &S) == 0 && S.n == 1);
  cjs_cut_range zero{0, 3}, back{5, 3};
  CHECK(ct_normalise(CJS_CUT_FIELDS, 9, &zero, 1, &S) == CJS_E_INVALID_ARG && ct_normalise(CJS_CUT_FIELDS, 9, &back, 1, &S) == CJS_E_INVALID_ARG);
  for (int round = 0; round < 3000; round++) {
    const uint32_t top = round % 3 == 0 ? 12 : (round % 3 == 1 ? 140 : 70);
    const Ranges r = random_ranges(top);
    CHECK(ct_normalise(round & 1, 9, r.data(), (uint32_t)r.size(), &S) == 0);
    CHECK(S.n >= 1 && S.n <= r.size() && S.beyond <= S.n);
    uint32_t lowest = ~0u;
    for (const cjs_cut_range& q : r) lowest = q.lo < lowest ? q.lo : lowest;
    CHECK(S.min_lo == lowest);
    for (uint32_t i = 0; i < S.n; i++) {
      CHECK(S.r[i].lo >= 1 && S.r[i].lo <= S.r[i].hi);
      if (i) CHECK(S.r[i - 1].hi != CT_TO_END && S.r[i - 1].hi + 1 < S.r[i].lo);      // sorted, disjoint, not touching
      CHECK((S.r[i].hi > 64) == (i >= S.beyond));
    }
    const CtView V = ct_view(S);
    for (uint32_t k = 1; k <= 2 * top + 70; k++) CHECK(ct_member(V, k) == naive_member(r, k));
    for (uint32_t k : {0xFFFFFFFEu, 0xFFFFFFFFu, 0x80000000u}) CHECK(ct_member(V, k) == naive_member(r, k));
  }
}

static std::string random_text(size_t n, uint8_t d) {
  const uint8_t alphabet[6] = {d, d, '\n', 'a', 'b', 'c'};
  const uint32_t kinds = below(3) ? 6 : 4;
  std::string s(n, 0);
  for (char& c : s) c = (char)alphabet[below(kinds)];
  return s;
}

static bool same_sum(const CtSum& a, const CtSum& b) { return a.nl == b.nl && a.units == b.units && a.flags == b.flags; }

static void check_monoid_and_pieces() {
  for (int round = 0; round < 2000; round++) {
    const uint32_t mode = round & 1;
    const uint8_t d = round % 5 == 0 ? 0 : (round % 7 == 0 ? 0xFF : ',');
    const std::string text = random_text(below(400), d);
    const uint8_t* p = (const uint8_t*)text.data();
    const size_t n = text.size(), i = below((uint32_t)n + 1), j = i + below((uint32_t)(n - i) + 1);
    const CtSum a = ct_summary(p, i, mode, d), b = ct_summary(p + i, j - i, mode, d), c = ct_summary(p + j, n - j, mode, d), whole = ct_summary(p, n, mode, d);
    CHECK(same_sum(ct_comb(ct_comb(a, b), c), whole) && same_sum(ct_comb(a, ct_comb(b, c)), whole));
    CHECK(same_sum(ct_comb(ct_none(), whole), whole) && same_sum(ct_comb(whole, ct_none()), whole));
    // what a summary says, counted naively
    const size_t last = text.rfind('\n');
    const std::string behind = last == std::string::npos ? text : text.substr(last + 1);
    uint64_t nls = 0; uint32_t units = 0;
    for (char ch : text) nls += ch == '\n';
    for (char ch : behind) units += mode == CJS_CUT_BYTES || (uint8_t)ch == d;
    CHECK(whole.nl == nls && whole.units == units && !!(whole.flags & CT_HAS_NL) == (last != std::string::npos) && !!(whole.flags & CT_ANY) == !behind.empty());

    // the pieces, each met in the state the ones in front left, against the whole: all lines, and a window of lines
    const Ranges r = random_ranges(round % 3 ? 6 : 80);
    CtSel S;
    CHECK(ct_normalise(mode, d, r.data(), (uint32_t)r.size(), &S) == 0);
    const CtView V = ct_view(S);
    std::vector<uint8_t> want(n + 1), got(n + 1);
    const size_t wn = cut_text(S, p, n, want.data(), want.size());
    CHECK(wn <= n + 1);
    CHECK(std::string((const char*)want.data(), wn) == naive_cut(text, mode, d, r));
    const uint64_t first = round % 4 ? 0 : below((uint32_t)nls + 2), end = round % 4 ? ~0ull : first + below((uint32_t)nls + 2);
    CtSum s = ct_none(), by_sum = ct_none();
    size_t w = 0;
    const size_t cuts[4] = {0, i, j, n};
    for (int k = 0; k < 3; k++) {
      CHECK(same_sum(s, by_sum));                       // the state in front of piece k is the scan of the summaries in front of it
      w += ct_piece(V, first, end, s, p + cuts[k], cuts[k + 1] - cuts[k], got.data() + w, got.size() - w);
      by_sum = ct_comb(by_sum, ct_summary(p + cuts[k], cuts[k + 1] - cuts[k], mode, d));
    }
    if (ct_tail_newline(s, first, end)) got[w++] = '\n';
    if (round % 4) CHECK(w == wn && !memcmp(got.data(), want.data(), wn));
    else {                                              // the window's lines cut out of the text: the same as cutting them alone
      std::string sub;
      uint64_t line = 0;
      for (char ch : text) { if (line >= first && line < end) sub.push_back(ch); line += ch == '\n'; }
      CHECK(std::string((const char*)got.data(), w) == naive_cut(sub, mode, d, r));
    }
    // a cap: the size all the same, nothing past the cap
    if (wn) {
      std::vector<uint8_t> small(wn, 0xA5);
      CHECK(cut_text(S, p, n, small.data(), wn - 1) == wn && small[wn - 1] == 0xA5 && !memcmp(small.data(), want.data(), wn - 1));
    }
  }
}

static void check_rule_per_byte() {
  // the rule as the contract states it per byte, against ct_step on one line
  for (int round = 0; round < 500; round++) {
    const Ranges r = random_ranges(8);
    CtSel S;
    CHECK(ct_normalise(CJS_CUT_FIELDS, ';', r.data(), (uint32_t)r.size(), &S) == 0);
    const CtView V = ct_view(S);
    CtSum s = ct_none();
    uint32_t field = 1;
    for (int i = 0; i < 40; i++) {
      const uint8_t ch = below(3) ? 'x' : ';';
      bool want;
      if (ch == ';') { field++; want = naive_member(r, field) && has_below(r, field); }
      else want = naive_member(r, field);
      CHECK(ct_step(V, 0, 1, s, ch) == want);
    }
    CHECK(ct_step(V, 0, 1, s, '\n') && s.nl == 1 && s.units == 0);
    CHECK(!ct_step(V, 0, 1, s, 'x') && !ct_step(V, 0, 1, s, '\n'));      // line 1 is outside the window: not even its newline
  }
}

static void check_saturation() {
  CHECK(ct_sat_add(CT_SAT, 1) == CT_SAT && ct_sat_add(CT_SAT - 1, 1) == CT_SAT && ct_sat_add(0x80000000u, 0x80000000u) == CT_SAT && ct_sat_add(3, 4) == 7);
  const cjs_cut_range all[2] = {{2, 2}, {0xFFFFFFF0u, CT_TO_END}};
  for (uint32_t mode : {CJS_CUT_FIELDS, CJS_CUT_BYTES}) {
    CtSel S;
    CHECK(ct_normalise(mode, ',', all, 2, &S) == 0);
    const CtView V = ct_view(S);
    CtSum s{5, CT_SAT - 2, CT_ANY};                     // deep inside a line of line number 5
    for (int i = 0; i < 6; i++) {
      CHECK(ct_step(V, 0, 9, s, ','));                  // units 0xFFFFFFFD .. : selected by the open range, and it stays so
      CHECK(s.units <= CT_SAT && s.nl == 5);
    }
    CHECK(s.units == CT_SAT);
    CtSum p{0, CT_SAT - 1, CT_ANY};
    for (int i = 0; i < 4; i++) ct_push(p, mode, ',', ',');
    CHECK(p.units == CT_SAT);
    // saturation is the same in the scan and in the walk: a piece behind a saturated piece
    const CtSum a{0, CT_SAT - 1, CT_ANY}, b{0, 5, CT_ANY}, c{0, 7, CT_ANY};
    CHECK(same_sum(ct_comb(ct_comb(a, b), c), ct_comb(a, ct_comb(b, c))) && ct_comb(a, b).units == CT_SAT);
  }
}

int main() {
  check_parser();
  check_normal_form_and_membership();
  check_monoid_and_pieces();
  check_rule_per_byte();
  check_saturation();
  if (fails) { printf("cut_plan_check: %d checks failed\n", fails); return 1; }
  printf("cut_plan_check ok\n");
  return 0;
}
