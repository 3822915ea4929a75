// bwt_rules_check.cc — the rules of the suffix sort, csrc/bwt_rules.h (window ownership of the tile sorters, the large-group test,
// the record layouts, the key arithmetic of round 1 and the stepping of the rounds), checked by property against a serial model of
// the grouping, not by restating the formulas: every window of a few thousand random group-size sequences is walked with the
// header's functions only, the way the two tile sorters walk it.
// Stand-alone: built with the host compiler under the address / undefined-behaviour sanitizers and run by
// tests/test_bwt_rules_host.py.  Exit 0 = all checks passed; a failing check prints itself and the program exits 1.
#include "bwt_rules.h"
#include <stdio.h>
#include <vector>

using namespace cjs;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
typedef unsigned long long ull;

// ---- the model: an array of A slots cut into groups; slot a carries the ordinal of its group (what gord[] holds in a round >= 2)
struct Groups {
  std::vector<uint32_t> start, size;      // per group
  std::vector<uint32_t> gord;             // per slot
  uint32_t A = 0;
  void add(uint32_t m) { start.push_back(A); size.push_back(m); gord.insert(gord.end(), m, (uint32_t)start.size() - 1u); A += m; }
};
static const uint32_t kSizes[] = {2, 3, 63, 64, 65, 1023, 1024, 1025, 3071, 3072, 3073, 5000};
// sizes from the list plus random ones; starts steered to -1, 0, +1 of multiples of TS_NOM; the array ends where asked
static Groups random_groups(uint32_t total) {
  Groups g;
  while (g.A < total) {
    const uint32_t left = total - g.A;
    uint32_t m;
    switch (rnd() % 4) {
      case 0: m = kSizes[rnd() % 12]; break;
      case 1: m = 1 + (uint32_t)(rnd() % 8); break;
      case 2: m = 1 + (uint32_t)(rnd() % 1400); break;
      default: {                            // a filler that makes the NEXT group start at -1, 0, +1 of a multiple of TS_NOM
        const uint32_t want = (g.A / TS_NOM + 1) * TS_NOM + (uint32_t)(rnd() % 3) - 1u;
        m = want - g.A;
        if (rnd() & 1) m = m > 700 ? 1 + (uint32_t)(rnd() % 700) : m;      // (in pieces, so that the filler itself is not always large)
      }
    }
    if (m == 0) m = 1;
    g.add(m < left ? m : left);
  }
  return g;
}

// ---- every window of g, walked with the header's functions only
static void check_windows(const Groups& g, int seq) {
  const uint32_t A = g.A, nwin = ts_windows(A);
  CHECK(nwin >= 1 && ts_win_base(nwin - 1) < A && (uint64_t)nwin * TS_NOM >= A, "seq %d: %u windows for A = %u", seq, nwin, A);
  std::vector<uint8_t> owners(A, 0), fetchers(A, 0);
  std::vector<uint32_t> owner_win(A, 0), fetch_win(A, 0);
  for (uint32_t win = 0; win < nwin; win++) {
    const uint64_t wb = ts_win_base(win);
    const uint32_t L = ts_win_len(wb, A);
    const bool at_end = wb + L == A;
    CHECK(L >= 1 && L <= TS_WIN && wb + L <= A && (L == TS_WIN || at_end), "seq %d window %u: L = %u", seq, win, L);
    uint64_t hm[64] = {0};
    for (uint32_t x = 0; x < L; x++)
      if (wb + x == 0 || g.gord[wb + x] != g.gord[wb + x - 1]) hm[x >> 6] |= 1ull << (x & 63);
    int wlast[64], wnext[64];               // what the wave scans of the kernels leave: last head before / first head behind each word
    for (int i = 0, last = TS_NO_HEAD; i < 64; i++) { wlast[i] = last; if (hm[i]) last = word_last(hm[i], i); }
    for (int i = 63, next = TS_NO_NEXT; i >= 0; i--) { wnext[i] = next; if (hm[i]) next = word_first(hm[i], i); }
    uint32_t li_max = 0;                    // the TS_MAXGRP ordinals in front of the window, four to a thread
    if (wb) for (uint32_t t = 0; t < TS_MAXGRP / 4; t++) {
      const uint32_t* q = &g.gord[wb - TS_MAXGRP + 4 * t];
      const uint32_t li = ts_li4(t, q[0], q[1], q[2], q[3], g.gord[wb]);
      if (li > li_max) li_max = li;
    }
    const uint32_t prev_end = ts_prev_end(wb, L, at_end, li_max, hm[0], wnext[0]);
    // the model: the group that holds slot wb, when it starts in front of the window and is small enough to have an owner
    const uint32_t g0 = g.gord[wb];
    const uint32_t want_prev = g.start[g0] < wb && g.size[g0] <= TS_MAXGRP ? (uint32_t)(g.start[g0] + g.size[g0] - wb) : 0u;
    CHECK(prev_end == want_prev, "seq %d window %u: prev_end %u, the model says %u", seq, win, prev_end, want_prev);
    for (uint32_t x = 0; x < TS_WIN; x++) {
      const int wi = (int)(x >> 6), lane = (int)(x & 63);
      const int hx = ts_head_of(hm[wi], wi, lane, wlast[wi]), nx = ts_next_of(hm[wi], wi, lane, wnext[wi]);
      const TsOwn own = ts_classify(hx, nx, L, at_end);
      const bool valid = x < L, owned = valid && own.owned;
      CHECK(!own.owned || own.small, "seq %d window %u slot %u: owned but not small", seq, win, x);
      CHECK(!own.medium || own.owned, "seq %d window %u slot %u: medium but not owned", seq, win, x);
      if (!valid) { CHECK(!ts_fetches(valid, x, prev_end, owned), "seq %d window %u: slot %u past L fetched", seq, win, x); continue; }
      const uint32_t gi = g.gord[wb + x];
      if (owned) {
        const int e = ts_close(nx, L, at_end);
        CHECK(wb + hx == g.start[gi] && (uint32_t)(e - hx) == g.size[gi], "seq %d window %u slot %u: owned as [%d, %d), the group is [%u, +%u)",
              seq, win, x, hx, e, g.start[gi], g.size[gi]);
        CHECK(hx >= 0 && e <= (int)L, "seq %d window %u slot %u: the owned group [%d, %d) leaves the window's %u slots", seq, win, x, hx, e, L);
        CHECK(own.medium == (g.size[gi] > TS_TINY), "seq %d window %u slot %u: medium = %d for %u members", seq, win, x, (int)own.medium, g.size[gi]);
        owners[wb + x]++; owner_win[wb + x] = win;
      }
      if (ts_fetches(valid, x, prev_end, owned)) { fetchers[wb + x]++; fetch_win[wb + x] = win; }
    }
  }
  for (uint32_t a = 0; a < A; a++) {
    const uint32_t gi = g.gord[a];
    const bool small = g.size[gi] <= TS_MAXGRP;
    CHECK(owners[a] == (small ? 1 : 0), "seq %d slot %u (group of %u at %u): %d owners", seq, a, g.size[gi], g.start[gi], (int)owners[a]);
    CHECK(!small || owner_win[a] == g.start[gi] / TS_NOM, "seq %d slot %u: owned by window %u, its head %u lies in window %u", seq, a, owner_win[a], g.start[gi], g.start[gi] / TS_NOM);
    CHECK(fetchers[a] == 1, "seq %d slot %u (group of %u at %u): %d windows fetch its rank", seq, a, g.size[gi], g.start[gi], (int)fetchers[a]);
    CHECK(fetch_win[a] == (small ? g.start[gi] : a) / TS_NOM, "seq %d slot %u: fetched by window %u", seq, a, fetch_win[a]);
  }
}

// ---- the large-group test: per 4096-slot tile as the three counting kernels apply it (eight mask words to a run; per wave of
// 1024 slots, 32 threads of 16 slots to a run), against "some aligned run of LG_RUN slots, wholly below A, holds no head"
static bool check_large_flag(const Groups& g, int seq) {
  const uint32_t A = g.A;
  bool flag = false, want = false, any_large = false;
  for (uint64_t k = 0; (k + 1) * LG_RUN <= A; k++) {
    bool head = false;
    for (uint64_t a = k * LG_RUN; a < (k + 1) * LG_RUN; a++) head |= a == 0 || g.gord[a] != g.gord[a - 1];
    want |= !head;
  }
  for (uint64_t base = 0; base < A; base += 4096) {
    uint64_t words = 0;
    bool waves = false;
    for (uint32_t wv = 0; wv < 4; wv++) {
      uint64_t threads = 0;
      for (uint32_t x = 0; x < 1024; x++) {
        const uint64_t a = base + wv * 1024 + x;
        if (a < A && (a == 0 || g.gord[a] != g.gord[a - 1])) { threads |= 1ull << (x >> 4); words |= 1ull << (wv * 16 + (x >> 6)); }
      }
      waves |= run_without_head(threads, 32, base + wv * 1024, A);
    }
    CHECK(run_without_head(words, 8, base, A) == waves, "seq %d tile at %llu: the word form and the thread form disagree", seq, (ull)base);
    flag |= waves;
  }
  CHECK(flag == want, "seq %d: large-group flag %d, the model says %d", seq, (int)flag, (int)want);
  uint32_t largest = 0;
  for (uint32_t m : g.size) { any_large |= m > TS_MAXGRP - 1; if (m > largest) largest = m; }
  CHECK(!any_large || flag, "seq %d: a group of more than %u slots and no flag", seq, TS_MAXGRP - 1);
  CHECK(!flag || largest > LG_RUN, "seq %d: the flag with no group above %u slots (largest %u)", seq, LG_RUN, largest);
  return flag;
}

static void check_window_rule() {
  const uint32_t ends[] = {0, 1, 2, 63, 64, 1023, 1024, 1025, 2000, 3071};      // A mod TS_NOM: array ends in and around a window's slack
  for (int seq = 0; seq < 3000; seq++) {
    const uint32_t total = (uint32_t)(rnd() % 12) * TS_NOM + (seq % 3 ? ends[rnd() % 10] : (uint32_t)(rnd() % TS_NOM));
    const Groups g = random_groups(total ? total : 1);
    check_windows(g, seq);
    check_large_flag(g, seq);
  }
  // every listed size at every alignment of its start in a window (mod TS_NOM would take long: mod 64 and around the borders)
  for (uint32_t m : kSizes) for (uint32_t off = 0; off < TS_NOM + 2; off += (off > 70 && off < TS_NOM - 70 ? 97 : 1)) {
    Groups g; g.add(TS_NOM); if (off) g.add(off); g.add(m); g.add(5);
    check_windows(g, 100000 + (int)m);
  }
  // the flag at every alignment of a group's start: always from TS_MAXGRP slots on; LG_RUN + 1 is the smallest size that can raise it
  for (uint32_t off = 0; off < 2 * LG_RUN; off++) for (uint32_t m : {LG_RUN, LG_RUN + 1, TS_MAXGRP - 1, TS_MAXGRP, TS_MAXGRP + 1}) {
    Groups g; for (uint32_t i = 0; i < off; i++) g.add(1);
    g.add(m); g.add(1);
    const bool flag = check_large_flag(g, 200000 + (int)m);
    CHECK(m >= TS_MAXGRP ? flag : m > LG_RUN || !flag, "group of %u at %u: flag %d", m, off, (int)flag);
    if (m == LG_RUN + 1 && off == LG_RUN - 1) CHECK(flag, "a group of %u slots from %u covers the aligned run behind its head: no flag", m, off);
  }
}

// ---- the record layouts: every field comes back, no field overlaps another
static void check_layouts() {
  const uint32_t max_pos = BWT_MAX_STRIDE - 1, max_rank = RANK_MASK;      // positions up to 2^20 - 3, rank keys up to 2^20 - 1
  CHECK(max_pos == (1u << 20) - 3 && max_rank == (1u << 20) - 1, "limits");
  CHECK((pk_record(~0ull, 0, 0) & pk_record(0, 1, 0)) == 0 && (pk_record(~0ull, 0, 0) & pk_record(0, 0, PK_POS_MASK)) == 0 &&
        (pk_record(0, 1, 0) & pk_record(0, 0, PK_POS_MASK)) == 0, "pk_record: fields overlap");
  const uint64_t f2[4] = {pk2_record(0xFFFF, 0, 0, 0), pk2_record(0, max_rank, 0, 0), pk2_record(0, 0, 255, 0), pk2_record(0, 0, 0, PK_POS_MASK)};
  for (int i = 0; i < 4; i++) for (int j = i + 1; j < 4; j++) CHECK((f2[i] & f2[j]) == 0, "pk2_record: fields %d and %d overlap", i, j);
  CHECK((f2[0] | f2[1] | f2[2] | f2[3]) == ~0ull, "pk2_record: the fields leave bits free");
  CHECK((val_carrying(PK_POS_MASK, 0) & val_carrying(0, 255)) == 0, "val: fields overlap");
  CHECK((round_key(~0u, 0) & round_key(0, RANK_MASK)) == 0, "round_key: fields overlap");
  CHECK((ts64_owned(4095, 0, 0) & ts64_owned(0, max_rank, 0)) == 0 && (ts64_owned(4095, 0, 0) & ts64_owned(0, 0, ~0u)) == 0 &&
        (ts64_owned(0, max_rank, 0) & ts64_owned(0, 0, ~0u)) == 0 && ts64_owned(4095, 0, 0) >> 52 == 4095, "ts64: fields overlap");
  CHECK((ts32_owned(4095, 0) & ts32_owned(0, max_rank)) == 0 && ts32_owned(4095, 0) >> RANK_BITS == 4095, "ts32: fields overlap");
  for (uint32_t pos = 0; pos <= max_pos; pos++) {
    const uint32_t rank = max_rank - pos, prev = pos & 255u, b01 = (pos * 2654435761u) >> 16, par = pos & 1u;
    const uint64_t bytes = ((uint64_t)b01 << 24 | pos) & 0xFFFFFFFFFFull;
    const uint64_t r1 = pk_record(bytes, par, pos);
    CHECK(pk_pos(r1) == pos && ((r1 >> PK_SHIFT) & 1u) == par && (r1 >> PK_KEY_LO) == bytes && ((r1 >> (PK_SHIFT + 1)) & 7u) == 0, "pk_record at %u", pos);
    const uint64_t r2 = pk2_record(b01, rank, prev, pos);
    CHECK(pk_pos(r2) == pos && pk2_prev((uint32_t)r2) == prev && (r2 >> 48) == b01 && ((r2 >> PK2_GSHIFT) & RANK_MASK) == rank &&
          (r2 >> PK2_GSHIFT) == (((uint64_t)b01 << RANK_BITS) | rank), "pk2_record at %u", pos);
    const uint32_t v = val_carrying(pos, prev);
    CHECK(pk_pos(v) == pos && val_prev(v) == prev, "val at %u", pos);
    const uint32_t ord = (uint32_t)rnd();
    const uint64_t k = round_key(ord, rank);
    CHECK(round_key_ordinal(k) == ord && round_key_rank(k) == rank, "round_key at %u", pos);
    const uint32_t hs = pos & 4095u, sfx = val_carrying(pos, prev);
    const uint64_t e = ts64_owned(hs, rank, sfx);
    CHECK(e >> 52 == hs && ((e >> 32) & RANK_MASK) == rank && (uint32_t)e == sfx && ts64_count_word(e, hs) == ((rank << 12) | hs), "ts64 at %u", pos);
    CHECK(ts64_other(hs) >> 52 == hs && ts64_other(hs) > ts64_owned(hs, max_rank - 1, ~0u), "ts64_other at %u", hs);
    const uint32_t c = ts32_owned(hs, rank);
    CHECK(c >> RANK_BITS == hs && (c & RANK_MASK) == rank && ts32_other(hs) >> RANK_BITS == hs && (ts32_other(hs) & RANK_MASK) == 0, "ts32 at %u", pos);
  }
  for (uint32_t prev = 0; prev < 256; prev++) CHECK(val_prev(val_carrying(max_pos, prev)) == prev && pk2_prev((uint32_t)pk2_record(0xFFFF, max_rank, prev, max_pos)) == prev, "byte %u", prev);
  // the flag byte from two sorted composites, 64 and 32 bits wide, and the flag bits of four bytes as a mask
  for (int i = 0; i < 20000; i++) {
    const uint32_t o = (uint32_t)rnd() & 4095u, r = (uint32_t)rnd() & RANK_MASK, o2 = rnd() & 1 ? o : (uint32_t)rnd() & 4095u, r2 = rnd() & 1 ? r : (uint32_t)rnd() & RANK_MASK;
    const uint8_t want = hf_byte(o != o2 || r != r2, o != o2);
    CHECK(hf_of_sorted(round_key(o, r), round_key(o2, r2)) == want && hf_of_sorted(ts32_owned(o, r), ts32_owned(o2, r2)) == want, "hf_of_sorted");
    const uint32_t word = (uint32_t)rnd();
    for (int bit = 0; bit < 2; bit++) {
      uint32_t m = 0;
      for (int j = 0; j < 4; j++) m |= ((word >> (8 * j + bit)) & 1u) << j;
      CHECK(hf_bits4(word, bit) == m, "hf_bits4(%08x, %d) = %x, want %x", word, bit, hf_bits4(word, bit), m);
    }
  }
  CHECK(hf_byte(true, false) == HF_NEW && hf_byte(false, true) == HF_OLD && (HF_NEW & HF_OLD) == 0, "flag bits");
}

// ---- round 1 and the stepping of the rounds
static void check_round_arithmetic() {
  for (uint32_t nb = 1; nb <= 70000; nb++) for (int cyclic = 0; cyclic < 2; cyclic++) for (int seg = 0; seg < 2; seg++) for (int var = 0; var < 2; var++) {
    if (var && (!cyclic || seg)) continue;      // VarGeom: cyclic and unsegmented only
    const Round1Keys k = round1_keys(nb, cyclic, seg, var);
    const int id_bits = bits_for(nb - 1), shift = var ? r1_hole_bit(k.nsym) + 1 : r1_block_shift(cyclic, k.nsym);
    CHECK(k.nsym >= 1 && k.nsym <= 7 && k.bits >= 1 && k.bits <= 64, "nb %u cyclic %d seg %d var %d: nsym %d bits %d", nb, cyclic, seg, var, k.nsym, k.bits);
    CHECK(shift == k.nsym * (cyclic ? 8 : 9) + var && ((uint64_t)(nb - 1) >> id_bits) == 0, "nb %u: shift %d", nb, shift);
    if (!seg) CHECK(shift + id_bits == k.bits, "nb %u cyclic %d var %d: block id at %d + %d bits, key of %d", nb, cyclic, var, shift, id_bits, k.bits);
    else CHECK(k.nsym == 7 && k.bits == 7 * (cyclic ? 8 : 9), "nb %u: segmented keys", nb);
    if (!seg && k.nsym < 7) CHECK((k.nsym + 1) * (cyclic ? 8 : 9) + var + id_bits > 64, "nb %u: room for another symbol", nb);
    if (var) CHECK(var_geom_admits(k.nsym) == ((uint64_t)(BWT_MAX_STRIDE - 1) < (1ull << r1_hole_bit(k.nsym))), "nb %u: VarGeom admitted = %d with %d symbols", nb, (int)var_geom_admits(k.nsym), k.nsym);
  }
  // the block counts at which the depth of round 1 over blocks of different lengths changes (tests/test_gpu_bwt_var.py runs a call
  // on either side of both): 7 symbols up to 128 blocks, 6 up to 32768, 5 beyond
  CHECK(round1_keys(128, true, false, true).nsym == 7 && round1_keys(129, true, false, true).nsym == 6, "VarGeom depth at 128 / 129 blocks");
  CHECK(round1_keys(32768, true, false, true).nsym == 6 && round1_keys(32769, true, false, true).nsym == 5, "VarGeom depth at 32768 / 32769 blocks");
  // (no block count up to 70,000 leaves fewer than five symbols, so the refusal itself, symbol count by symbol count:)
  for (int nsym = 0; nsym <= 7; nsym++) CHECK(var_geom_admits(nsym) == ((uint64_t)(BWT_MAX_STRIDE - 1) < (1ull << r1_hole_bit(nsym))), "VarGeom with %d symbols", nsym);
  for (int b = 0; b <= 64; b++) for (int d = -1; d <= 1; d++) {
    const uint64_t x = (b == 64 ? 0 : 1ull << b) + (uint64_t)d;
    const int n = bits_for(x);
    CHECK(n >= 0 && n <= 64 && (n == 64 || x >> n == 0) && (n == 0 || x >> (n - 1) == 1), "bits_for(%llu) = %d", (ull)x, n);
  }
  for (int i = 0; i < 100000; i++) {
    const uint32_t ng = i < 64 ? (i < 32 ? 1u << i : ~0u >> (i - 32)) : (uint32_t)rnd() >> (rnd() % 32);
    const int bits = round_key_bits(ng);
    CHECK(bits >= RANK_BITS && bits <= 64 && (ng == 0 || round_key(ng - 1, RANK_MASK) >> bits == 0 || bits == 64), "round_key_bits(%u) = %d", ng, bits);
    const uint32_t A = (uint32_t)rnd() >> (rnd() % 32);
    CHECK(radix_tile_sorter(A, ng) == (ng != 0 && (uint64_t)A >= 5ull * ng), "radix_tile_sorter(%u, %u)", A, ng);
    CHECK(tile_sorted_round(A) == (A >= 2 * TS_WIN), "tile_sorted_round(%u)", A);
    CHECK(deferred_overflow(A, 2ull * ng) == (A > ng), "deferred_overflow(%u, %llu)", A, 2ull * ng);
  }
  for (uint32_t h0 = 1; h0 <= 7; h0++) {
    uint32_t h = h0;
    for (int i = 0; i < 64; i++) { const uint32_t n = next_depth(h); CHECK(n == (h < (1u << 29) ? 2 * h : h) && n >= h && n < (1u << 30), "next_depth(%u) = %u", h, n); h = n; }
    CHECK(h >= BWT_MAX_STRIDE, "depth from %u stops at %u, below a block's length", h0, h);
  }
  CHECK(bwt_admits(BWT_MAX_SLOTS - 1, BWT_MAX_STRIDE) && !bwt_admits(BWT_MAX_SLOTS, 1) && !bwt_admits(1, BWT_MAX_STRIDE + 1), "bwt_admits");
  CHECK(BWT_MAX_SLOTS - 1 + TS_WIN <= 0xFFFFFFFFull && BWT_MAX_STRIDE + 1 <= RANK_MASK, "limits: a window past the last slot, rank + 1 in 20 bits");
  CHECK(TS_NOM + TS_MAXGRP == TS_WIN && TS_WIN == 64 * 64 && LG_RUN * 2 == TS_MAXGRP && TS_GT * 2 == TS_WIN, "window constants");
  CHECK(CN_SURVIVORS == 0 && CN_GROUPS == 1 && CN_DEFERRED == 2 && CN_DEFERRED_GROUPS == 3 && CN_LARGE_GROUP == 4, "counter slots");
}

int main() {
  check_window_rule();
  check_layouts();
  check_round_arithmetic();
  if (g_fail) { printf("bwt_rules_check: %d checks FAILED\n", g_fail); return 1; }
  printf("bwt_rules_check ok\n");
  return 0;
}
