// tally_plan_check.cc -- the rule of the key tally (csrc/tally_plan.h) against a naive std::map, on the CPU: random key lists under
// both orders and the filters, records that differ in exactly one field, bad records left out, the count query and short caps, the
// argument errors, the bits of the order sort, and the newline join of a tail line against the key of the text with a newline
// appended.  A stand-alone program: it is built with the host compiler under the address and undefined-behaviour sanitizers and run
// (tests/test_tally_plan_host_check.py).
#include "tally_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include <tuple>
#include <vector>

using namespace cjs;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); if (++fails > 20) exit(1); } } while (0)

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static uint32_t below(uint32_t n) { return rnd() % n; }

typedef std::tuple<uint64_t, uint32_t, uint32_t> Rec;
struct Group { Rec rec; uint64_t first, count; };

// the naive table: a map from the record to (first, count), then the filter and a sort by the order's own words
static std::vector<Group> naive(const std::vector<cjs_bz_linekey>& keys, uint32_t order, uint64_t lo, uint64_t hi, cjs_tally_info& info) {
  std::map<Rec, std::pair<uint64_t, uint64_t>> m;
  info = cjs_tally_info{keys.size(), 0, 0, 0, 0};
  for (size_t i = 0; i < keys.size(); i++) {
    const cjs_bz_linekey& k = keys[i];
    if (k.hash == ~0ull && k.len == ~0u && k.check == ~0u) { info.n_bad++; continue; }
    auto it = m.find(Rec(k.hash, k.len, k.check));
    if (it == m.end()) m[Rec(k.hash, k.len, k.check)] = {i, 1}; else it->second.second++;
  }
  std::vector<Group> g;
  for (auto& e : m) {
    info.n_distinct++;
    if (e.second.second > info.max_count) info.max_count = e.second.second;
    if (e.second.second >= lo && (hi == 0 || e.second.second <= hi)) g.push_back(Group{e.first, e.second.first, e.second.second});
  }
  info.n_groups = g.size();
  for (size_t i = 1; i < g.size(); i++)      // insertion sort: by count descending then first, or by first
    for (size_t j = i; j > 0; j--) {
      const Group &a = g[j - 1], &b = g[j];
      const bool swap = order == CJS_TALLY_BY_COUNT ? (a.count < b.count || (a.count == b.count && a.first > b.first)) : a.first > b.first;
      if (!swap) break;
      std::swap(g[j - 1], g[j]);
    }
  return g;
}

static bool same_info(const cjs_tally_info& a, const cjs_tally_info& b) {
  return a.n_keys == b.n_keys && a.n_bad == b.n_bad && a.n_distinct == b.n_distinct && a.n_groups == b.n_groups && a.max_count == b.max_count;
}

static void check_list(const std::vector<cjs_bz_linekey>& keys) {
  static const uint64_t filters[][2] = {{1, 0}, {0, 0}, {2, 0}, {1, 1}, {2, 3}, {3, 3}, {1000000, 0}};
  for (uint32_t order = 0; order < 2; order++)
    for (auto& f : filters) {
      cjs_tally_info want, got;
      const std::vector<Group> g = naive(keys, order, f[0], f[1], want);
      const size_t caps[] = {keys.size() + 1, g.size(), g.size() ? g.size() - 1 : 0, 1, 0};
      for (size_t cap : caps) {
        std::vector<cjs_bz_tally> out(cap + 1);
        memset(out.data(), 0xA5, sizeof(cjs_bz_tally) * out.size());
        CHECK(tl_tally_host(keys.data(), keys.size(), order, f[0], f[1], cap ? out.data() : nullptr, cap, &got) == 0);
        CHECK(same_info(want, got));
        const size_t m = cap < g.size() ? cap : g.size();
        for (size_t i = 0; i < m; i++)
          CHECK(Rec(out[i].key.hash, out[i].key.len, out[i].key.check) == g[i].rec && out[i].first == g[i].first && out[i].count == g[i].count);
        const unsigned char* behind = (const unsigned char*)(out.data() + m);
        for (size_t i = 0; i < sizeof(cjs_bz_tally) * (out.size() - m); i++) if (behind[i] != 0xA5) { CHECK(!"written past the groups"); break; }
      }
    }
}

int main() {
  // random lists over records that collide field by field, some of them bad
  for (int round = 0; round < 400; round++) {
    const uint32_t n = round < 8 ? (uint32_t)round : below(400), pool = 1 + below(40), bad_in = below(4) ? 0 : 1 + below(8);
    std::vector<cjs_bz_linekey> vals(pool), keys(n);
    for (auto& v : vals) v = cjs_bz_linekey{(uint64_t)below(3) << 60 | below(3), below(3), below(3) << 31};
    for (auto& k : keys) k = bad_in && below(bad_in + 3) == 0 ? lk_bad_key() : vals[below(pool) % (1 + below(pool))];
    check_list(keys);
  }
  // records that differ in exactly one field are different groups; records that are all-ones in two fields are records, not bad
  {
    const cjs_bz_linekey base{5, 7, 9};
    std::vector<cjs_bz_linekey> keys = {base, {6, 7, 9}, {5, 8, 9}, {5, 7, 10}, base, {5 | 1ull << 60, 7, 9}, {~0ull, ~0u, 9}, {~0ull, 7, ~0u}, {5, ~0u, ~0u},
                                        lk_bad_key(), {~0ull, ~0u, 9}};
    cjs_tally_info info;
    std::vector<cjs_bz_tally> out(keys.size());
    CHECK(tl_tally_host(keys.data(), keys.size(), CJS_TALLY_BY_FIRST, 1, 0, out.data(), out.size(), &info) == 0);
    CHECK(info.n_bad == 1 && info.n_distinct == 8 && info.n_groups == 8 && info.max_count == 2);
    CHECK(out[0].first == 0 && out[0].count == 2 && out[5].first == 6 && out[5].count == 2);
    check_list(keys);
    CHECK(tl_less(base, keys[1]) && tl_less(base, keys[2]) && tl_less(base, keys[3]) && !tl_less(base, base) && tl_equal(base, keys[4]) && !tl_equal(base, keys[3]));
    CHECK(tl_less(cjs_bz_linekey{5, 9, 0}, cjs_bz_linekey{6, 0, 0}) && tl_less(cjs_bz_linekey{5, 1, 9}, cjs_bz_linekey{5, 2, 0}));      // hash, then len, then check
    for (const cjs_bz_linekey& k : keys) CHECK(lk_is_bad(k) || tl_less(k, lk_bad_key()));      // the bad record sorts behind every other
  }
  // only bad records; nothing at all
  {
    std::vector<cjs_bz_linekey> keys(5, lk_bad_key());
    cjs_tally_info info;
    cjs_bz_tally one;
    CHECK(tl_tally_host(keys.data(), 5, CJS_TALLY_BY_COUNT, 1, 0, &one, 1, &info) == 0 && info.n_bad == 5 && info.n_distinct == 0 && info.n_groups == 0 && info.max_count == 0);
    CHECK(tl_tally_host(nullptr, 0, CJS_TALLY_BY_COUNT, 1, 0, nullptr, 0, &info) == 0 && info.n_keys == 0 && info.n_groups == 0);
  }
  // the argument errors
  {
    cjs_bz_linekey k{1, 2, 3};
    cjs_bz_tally o;
    cjs_tally_info info;
    CHECK(tl_tally_host(&k, 1, 0, 1, 0, &o, 1, nullptr) == CJS_E_INVALID_ARG);
    CHECK(tl_tally_host(nullptr, 1, 0, 1, 0, &o, 1, &info) == CJS_E_INVALID_ARG);
    CHECK(tl_tally_host(&k, 1, 0, 1, 0, nullptr, 1, &info) == CJS_E_INVALID_ARG);
    CHECK(tl_tally_host(&k, 1, 2, 1, 0, &o, 1, &info) == CJS_E_INVALID_ARG);
    CHECK(tl_tally_host(&k, 1, 0, 3, 2, &o, 1, &info) == CJS_E_INVALID_ARG);
    CHECK(tl_tally_host(&k, 1, 0, 3, 3, &o, 1, &info) == 0 && tl_tally_host(&k, 1, 1, 0, 0, &o, 1, &info) == 0);
    CHECK(tl_tally_host(&k, (size_t)TL_MAX_KEYS + 1, 0, 1, 0, nullptr, 0, &info) == CJS_E_UNSUPPORTED);      // (refused before a key is read)
  }
  // the order words, and the bits of them that can differ
  {
    CHECK(tl_order_word(CJS_TALLY_BY_FIRST, 77, 5) == 77 && tl_order_word(CJS_TALLY_BY_COUNT, 77, 5) == (0xFFFFFFFAull << 32 | 77));
    CHECK(tl_order_bits(CJS_TALLY_BY_FIRST, 1u << 30) == 32 && tl_order_bits(CJS_TALLY_BY_COUNT, 1) == 40 && tl_order_bits(CJS_TALLY_BY_COUNT, 255) == 40);
    CHECK(tl_order_bits(CJS_TALLY_BY_COUNT, 256) == 48 && tl_order_bits(CJS_TALLY_BY_COUNT, 0xFFFFFFFEull) == 64);
    for (int i = 0; i < 2000; i++) {      // two words of counts up to max_count agree above the covered bits
      const uint64_t mc = 1 + (rnd() >> below(31)), a = 1 + rnd() % mc, b = 1 + rnd() % mc;
      const int bits = tl_order_bits(CJS_TALLY_BY_COUNT, mc);
      if (bits < 64) CHECK(tl_order_word(CJS_TALLY_BY_COUNT, rnd(), a) >> bits == tl_order_word(CJS_TALLY_BY_COUNT, rnd(), b) >> bits);
    }
  }
  // the tail line's key: the open fragment joined with the fragment of "\n" is the key of the text with a newline appended
  for (int round = 0; round < 300; round++) {
    const LkBases B = lk_bases(round * 0x9E37ull);
    std::string text;
    for (uint32_t i = below(round < 5 ? 1 : 200); i > 0; i--) text.push_back((char)(below(4) ? 'a' + below(3) : below(256)));
    for (char& c : text) if (c == '\n') c = 'n';
    LkFrag open{0, 0, 0}, whole{0, 0, 0};
    for (char c : text) lk_push(open, B, (uint8_t)c);
    for (char c : text + "\n") lk_push(whole, B, (uint8_t)c);
    const cjs_bz_linekey a = lk_key(tl_join_newline(open, B)), b = lk_key(whole);
    CHECK(tl_equal(a, b) && a.len == text.size() + 1);
  }
  if (fails) { printf("tally_plan_check: %d failures\n", fails); return 1; }
  printf("tally_plan_check ok\n");
  return 0;
}
